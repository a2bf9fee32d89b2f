#!/usr/bin/env python3
"""Colour input (sdvl_convert_gray, to_gray_kernel) in isolation, and the farm on colour frames next to the same frames in gray.
    python tools/color_bench.py kernel [n_frames] [reps]     dispatch time of to_gray per n 640x480 frames from HBM and from pinned
                                                          host memory, RGB and RGBA -> bytes / s (read C W H + write W H per frame)
    python tools/color_bench.py farm [G] [Bg] [steps]       tracked frames / s of a farm on resident RGB frames vs their gray
Run `kernel` under `rocprofv3 --kernel-trace --stats -- python tools/color_bench.py kernel` for the profiler's view of the same launches."""
import ctypes as C
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

sdvl = importlib.import_module("slam-sdvl_amd")
W, H = 640, 480


def kernel(n, reps):
    ctx = sdvl.Context(0)
    lib = ctx.lib
    lib.sdvl_convert_gray.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    rng = np.random.default_rng(1)
    dst_buf = ctx.device_malloc(n * W * H)
    dst = (C.c_void_p * n)(*[dst_buf + i * W * H for i in range(n)])
    for ch, fmt in ((3, sdvl.SDVL_RGB8), (4, sdvl.SDVL_RGBA8)):
        fb = W * H * ch
        import torch
        host = rng.integers(0, 256, n * fb, dtype=np.uint8)
        dev_t = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        dev = dev_t.data_ptr()
        pinned = C.c_void_p()
        ctx._check(lib.sdvl_host_alloc_pinned(ctx.h, C.c_int64(n * fb), C.byref(pinned)))
        C.memmove(pinned.value, host.ctypes.data, n * fb)
        for where, base, on_dev in (("hbm", dev, 1), ("pinned", pinned.value, 0)):
            src = (C.c_void_p * n)(*[base + i * fb for i in range(n)])
            for _ in range(2):
                ctx._check(lib.sdvl_convert_gray(ctx.h, n, src, W * ch, on_dev, W, H, fmt, dst, W))
            ctx.synchronize()
            ctx.timing_enable(True)
            ctx.timing_reset()
            for _ in range(reps):
                ctx._check(lib.sdvl_convert_gray(ctx.h, n, src, W * ch, on_dev, W, H, fmt, dst, W))
            ctx.synchronize()
            ms, launches = ctx.timing_get()["to_gray"]
            ctx.timing_enable(False)
            per = ms / launches
            gbs = n * (ch + 1) * W * H / (per * 1e-3) / 1e9
            print("to_gray %-4s from %-6s: %d frames %8.1f us  %7.1f GB/s (read %d B + write 1 B per pixel)" %
                  ("RGB" if ch == 3 else "RGBA", where, n, per * 1e3, gbs, ch))
        ctx._check(lib.sdvl_host_free_pinned(ctx.h, pinned))
        del dev_t
    ctx.device_free(dst_buf)
    ctx.close()


def farm(G, Bg, steps):
    import torch
    import oraclelib as ol
    from test_color_cpu import to_gray
    trk = importlib.import_module("slam-sdvl_amd.tracker")
    trk.configure()
    syn, orc = ol.Synth(), ol.Oracle()
    N = G * Bg
    # N sequences of `steps` frames, rendered once on the host; colour = gray + seeded per-channel offsets
    rng = np.random.default_rng(3)
    off = rng.integers(-30, 31, (N, 1, 1, 3))
    base = [[syn.render(ol.trajectory_pose(orc, k, ol.XI * (1.0 + 0.01 * (i % 16))), ol.TUM_CAM, W, H, seed=20260001 + i % 16, frame_id=k)
             for k in range(steps)] for i in range(min(N, 16))]
    col = np.empty((steps, N, H, W, 3), np.uint8)
    for k in range(steps):
        for i in range(N):
            col[k, i] = np.clip(base[i % 16][k][..., None].astype(np.int32) + off[i], 0, 255)
    gray = to_gray(col, "rgb")
    for fmt, data in (("gray", gray), ("rgb", col), ("gray", gray), ("rgb", col)):
        d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        torch.cuda.synchronize()
        fb = data[0, 0].nbytes
        ptrs = np.array([[d.data_ptr() + (k * N + i) * fb for i in range(N)] for k in range(steps)], np.uint64)
        f = trk.TrackerFarm(0, G, Bg, W, H, ol.TUM_CAM)
        f.reserve(steps // 4 + 8)
        f.set_color(fmt)
        f.run(ptrs[:2])          # warm-up (bootstrap steps)
        f.close()
        f = trk.TrackerFarm(0, G, Bg, W, H, ol.TUM_CAM)
        f.reserve(steps // 4 + 8)
        f.set_color(fmt)
        out = f.alloc_stats(steps)
        t0 = time.perf_counter()
        f.run(ptrs, out=out)
        dt = time.perf_counter() - t0
        tracked = sum(1 for o in out[G * Bg:] if o.quality != 2)   # (step 0: the bootstrap keyframes)
        print("farm %-4s G=%d Bg=%d steps=%d: %8.0f tracked frames/s (%d tracked in %.3f s)" % (fmt, G, Bg, steps, tracked / dt, tracked, dt))
        f.close()
        del d


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what == "kernel":
        kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 256, int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    else:
        farm(*(int(a) for a in sys.argv[2:5]))
