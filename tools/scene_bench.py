#!/usr/bin/env python3
"""Device time of the synthetic renderers for n views of 640x480 (default 256): the plane kernel (sdvl_synth_render), the scene kernel
(sdvl_synth_render_scene) with one unbounded surface — the same image — and with the four surfaces of `shelf`, image only and with
the depth and surface-id outputs.
    python tools/scene_bench.py [n_views] [rounds]
Each figure is the span between two HIP events on the context's stream around one call (record push + kernel; the calls wait for the
stream themselves), after a warm-up call of each form; the forms alternate inside every round and the median over the rounds is
printed with the spread.  The scene kernel's own dispatch time (events on its AQL packet, sdvl_ctx_timing_get) is printed beside it."""
import ctypes as C
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

sdvl = importlib.import_module("slam-sdvl_amd")
W, H = 640, 480
CAM = (517.3, 516.5, 318.6, 255.3)
XI = np.array([0.004, 0.002, 0.001, 0.0008, -0.0012, 0.0005])


def main(n, rounds):
    import oraclelib as ol
    orc = ol.Oracle()
    ctx = sdvl.Context(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0
    stream = C.c_void_p(ctx.stream())

    poses = [ol.trajectory_pose(orc, k % 64, XI * (1.0 + 0.01 * (k // 64))) for k in range(n)]
    views = []
    for k, T in enumerate(poses):
        v = sdvl.SynthView()
        s = sdvl.synth_scene(T, CAM, frame_id=k)
        v.fx, v.fy, v.u0, v.v0 = CAM
        for i in range(9):
            v.R[i] = s.R[i]
        for i in range(3):
            v.t[i] = s.t[i]
        v.plane[0], v.plane[1], v.plane[2], v.plane[3] = 0.0, 0.0, 1.0, 2.0
        v.seed, v.frame_id, v.texture = s.seed, k, 0
        views.append(v)
    one = [sdvl.synth_scene(T, CAM, frame_id=k) for k, T in enumerate(poses)]
    for s in one:
        s.n_surfaces = 1
        s.surfaces[0].plane[2], s.surfaces[0].plane[3] = 1.0, 2.0
        s.surfaces[0].e1[0], s.surfaces[0].e2[1] = 1.0, 1.0
    shelf = [sdvl.synth_scene(T, CAM, preset="shelf", frame_id=k) for k, T in enumerate(poses)]

    img = ctx.device_malloc(n * W * H)
    depth = ctx.device_malloc(4 * n * W * H)
    surf = ctx.device_malloc(n * W * H)
    forms = [("plane kernel", lambda: ctx.synth_render(views, W, H, img)),
             ("scene kernel, 1 surface", lambda: ctx.synth_render_scene(one, W, H, img)),
             ("scene kernel, shelf (4 surfaces)", lambda: ctx.synth_render_scene(shelf, W, H, img)),
             ("scene kernel, shelf + depth + ids", lambda: ctx.synth_render_scene(shelf, W, H, img, dev_depth=depth, dev_surface=surf))]
    ref = None
    for name, call in forms[:2]:                      # warm-up, and the one-surface scene is the plane scene
        call()
        got = ctx.device_download(img, n * W * H)
        assert ref is None or np.array_equal(got, ref), "the one-surface scene differs from the plane kernel"
        ref = got
    for _, call in forms[2:]:
        call()
    times = {name: [] for name, _ in forms}
    dispatch = {name: [] for name, _ in forms[1:]}
    ms = C.c_float()
    ctx.timing_enable(True)
    for _ in range(rounds):
        for name, call in forms:
            ctx.timing_reset()
            assert hip.hipEventRecord(ev[0], stream) == 0
            call()
            assert hip.hipEventRecord(ev[1], stream) == 0 and hip.hipEventSynchronize(ev[1]) == 0
            assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            times[name].append(ms.value)
            t = ctx.timing_get().get("synth_render_scene")
            if t and name in dispatch:
                dispatch[name].append(t[0] / max(1, t[1]))
    ctx.timing_enable(False)
    base = float(np.median(times[forms[0][0]]))
    for name, _ in forms:
        t = np.array(times[name])
        d = (", kernel dispatch %.3f ms" % np.median(dispatch[name])) if dispatch.get(name) else ""
        print("%-36s %d views %dx%d: median %.3f ms (min %.3f, max %.3f, %d rounds) = %.2f x the plane kernel, %.1f Gpixel/s%s" %
              (name, n, W, H, np.median(t), t.min(), t.max(), rounds, np.median(t) / base, n * W * H / np.median(t) / 1e6, d))
    for p in (img, depth, surf):
        ctx.device_free(p)
    for e in ev:
        hip.hipEventDestroy(e)
    ctx.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 256, int(sys.argv[2]) if len(sys.argv) > 2 else 9)
