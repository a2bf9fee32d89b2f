#!/usr/bin/env python3
"""Colour and raw camera input (sdvl_convert_gray: to_gray_kernel, bayer_gray_kernel, wide_gray_kernel) in isolation, and the farm on
colour and Bayer frames next to the same frames in gray.
    python tools/color_bench.py kernel [n_frames] [reps]     dispatch time per n 640x480 frames from HBM and from pinned host memory, RGB
                                                          and RGBA and every raw format, alternated within the process -> bytes / s
                                                          (read bpp W H + write W H per frame; a Bayer source in host memory is staged
                                                          by a copy first: its line also gives the wall time per call, copy included)
    python tools/color_bench.py farm [G] [Bg] [steps]       tracked frames / s of a farm on resident RGB frames vs their gray
    python tools/color_bench.py bayer [G] [Bg] [steps] [rounds]   the same on Bayer (RGGB) frames, resident and host-fed through the
                                                          input ring, beside the gray run of the same session (alternated, `rounds` times
                                                          each, default 2: the rounds show the run-to-run spread)
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
    import torch
    formats = (("RGB", 3, sdvl.SDVL_RGB8, "to_gray"), ("RGBA", 4, sdvl.SDVL_RGBA8, "to_gray"), ("BAYER", 1, sdvl.SDVL_BAYER_RGGB8, "bayer_gray"),
               ("YUYV", 2, sdvl.SDVL_YUYV8, "wide_gray"), ("GRAY12", 2, sdvl.SDVL_GRAY12_16, "wide_gray"), ("GRAY16", 2, sdvl.SDVL_GRAY16, "wide_gray"))
    for name, ch, fmt, key in formats * 2:   # every format twice, alternated: the second round shows the run-to-run spread
        fb = W * H * ch
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
            ms, launches = ctx.timing_get()[key]
            ctx.timing_enable(False)
            per = ms / launches
            gbs = n * (ch + 1) * W * H / (per * 1e-3) / 1e9
            t0 = time.perf_counter()
            for _ in range(reps):
                ctx._check(lib.sdvl_convert_gray(ctx.h, n, src, W * ch, on_dev, W, H, fmt, dst, W))
            ctx.synchronize()
            wall = (time.perf_counter() - t0) / reps
            print("%-10s %-6s from %-6s: %d frames %8.1f us  %7.1f GB/s (read %d B + write 1 B per pixel)  call %8.1f us wall" %
                  (key, name, where, n, per * 1e3, gbs, ch, wall * 1e6))
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


def bayer(G, Bg, steps, rounds=2):
    """the farm on RGGB mosaics and on their restated gray, resident in HBM and host-fed (pinned memory, input ring)"""
    import torch
    import oraclelib as ol
    import raw_restatement as raw
    trk = importlib.import_module("slam-sdvl_amd.tracker")
    trk.configure()
    syn, orc = ol.Synth(), ol.Oracle()
    N, D = G * Bg, min(G * Bg, 16)
    rng = np.random.default_rng(3)
    off = rng.integers(-30, 31, (D, 1, 1, 3))
    # D distinct sequences, rendered once on the host; sequence i of the farm follows i mod D
    mos = np.empty((steps, D, H, W), np.uint8)
    for i in range(D):
        for k in range(steps):
            g = syn.render(ol.trajectory_pose(orc, k, ol.XI * (1.0 + 0.01 * i)), ol.TUM_CAM, W, H, seed=20260001 + i, frame_id=k)
            mos[k, i] = raw.bayer_sample(np.clip(g[..., None].astype(np.int32) + off[i], 0, 255).astype(np.uint8), "bayer_rggb")
    gray = np.stack([raw.bayer_to_gray(mos[k], "bayer_rggb") for k in range(steps)])
    fb = W * H
    which = np.arange(N, dtype=np.uint64) % D
    idx = np.arange(steps, dtype=np.uint64)[:, None] * D + which[None, :]
    pinned = torch.empty(steps * D * fb, dtype=torch.uint8, pin_memory=True)
    for fmt, data, fed in [(f, d, w) for _ in range(rounds) for w in ("resident", "host-fed") for f, d in (("gray", gray), ("bayer_rggb", mos))]:
        if fed == "resident":
            d = torch.from_numpy(data.reshape(-1)).cuda()
            torch.cuda.synchronize()
            base = d.data_ptr()
        else:
            pinned.numpy()[:] = data.reshape(-1)
            base = pinned.data_ptr()
        ptrs = (base + idx * fb).astype(np.uint64)
        for timed in (False, True):   # a warm-up farm over the bootstrap steps, then the timed one
            f = trk.TrackerFarm(0, G, Bg, W, H, ol.TUM_CAM)
            f.reserve(steps // 4 + 8)
            f.set_color(fmt)
            f.set_host_input(fed == "host-fed")
            if not timed:
                f.run(ptrs[:2])
            else:
                out = f.alloc_stats(steps)
                t0 = time.perf_counter()
                f.run(ptrs, out=out)
                dt = time.perf_counter() - t0
                tracked = sum(1 for o in out[N:] if o.quality != 2)   # (step 0: the bootstrap keyframes)
                print("farm %-10s %-8s G=%d Bg=%d steps=%d: %8.0f tracked frames/s (%d tracked in %.3f s)" %
                      (fmt, fed, G, Bg, steps, tracked / dt, tracked, dt))
            f.close()
        d = None


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    if what == "kernel":
        kernel(int(sys.argv[2]) if len(sys.argv) > 2 else 256, int(sys.argv[3]) if len(sys.argv) > 3 else 20)
    elif what == "bayer":
        bayer(*(int(a) for a in sys.argv[2:6]))
    else:
        farm(*(int(a) for a in sys.argv[2:5]))
