"""The depth plane written on the caller's stream (tests/test_gpu_depth_test.py), as a program of its own: torch must initialise its HIP
runtime BEFORE libgs4d.so is loaded into the process (as bench.py does).

The caller rewrites the plane through its device pointer on ITS stream before every frame (gs4d_buffer_device_ptr + gs4d_buffer_invalidate),
renders, and reads the frame back on the device (gs4d_read_pixels_device) into a tensor it consumes on its stream (gs4d_set_stream) — frame
after frame, lanes in flight.  Exit code 0 = every frame is bit-equal to its twin: the same frame without the test, with alpha 0 for every
record the plane hides (tests/ztest_cases.py), rendered by a second context.  The draw path comes from the environment."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
torch.cuda.init()
import scenes                     # noqa: E402
import ztest_cases as zc          # noqa: E402


def main():
    side = torch.cuda.Stream()
    gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.restype = C.c_int
    n, W, H = 100_000, 640, 360
    cam = scenes.CAM_CUBE
    view = gs4d.look_at(cam[0], cam[1])
    proj = gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR)
    pos, q, sc, rgba = scenes.cube_params(n, seed=71)
    rec = gs4d.build_records_3d(pos, q, sc * 2.0, rgba)

    def setup(ctx, data):
        db, kb, ib = ctx.buffer(data), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
        ctx.set_clear_color(gs4d.CLEAR_COLOR)
        ctx.set_uniforms(time=0.0, min_opacity=0.0, view=view, proj=proj)
        return db, kb, ib

    def draw(ctx, b):
        ctx.keygen(b[0], 0.0, cam[0], b[1], b[2], n)
        ctx.sort_pairs(b[1], b[2], n)
        ctx.set_mode(gs4d.MODE_4D_SORTED)
        ctx.bind(1, b[2])
        ctx.bind(2, b[0])
        ctx.draw_instanced(n)

    # record depths: slot 15 of an aux frame
    ref = gs4d.Context(W, H)
    ref.set_aux_outputs(True)
    b = setup(ref, rec)
    ref.clear()
    draw(ref, b)
    pj = ref.debug_projected(n)
    d, valid = pj[:, 15].copy(), pj[:, 14] != 0
    zs = zc.pick_thresholds(d[valid])
    seq = [zs[0], zs[2], zs[1], np.float32(np.inf), zs[2], zs[0]]
    twins = {}
    for z in set(seq):
        ref.subdata(b[0], zc.hide_alpha(rec, d, z, 7))
        ref.clear()
        draw(ref, b)
        twins[z] = ref.read_pixels()
    ref.close()

    ctx = gs4d.Context(W, H)
    b = setup(ctx, rec)
    ctx.set_stream(side.cuda_stream)
    plane = ctx.buffer(nbytes=4 * W * H)
    pptr, nbytes = ctx.device_ptr(plane)
    assert nbytes == 4 * W * H
    ctx.set_depth_test(plane)
    outs, keep = [], []
    with torch.cuda.stream(side):
        for z in seq:
            src = torch.full((H * W,), float(z), dtype=torch.float32, device="cuda")
            keep.append(src)
            ctx.invalidate(plane)                                   # the side stream now waits for the frames that still read the plane
            assert hip.hipMemcpyAsync(pptr, src.data_ptr(), 4 * W * H, 3, C.c_void_p(side.cuda_stream)) == 0
            ctx.clear()
            draw(ctx, b)
            ff = torch.empty(H * W * 4, dtype=torch.float32, device="cuda")
            ctx.read_pixels_device(ff.data_ptr(), ff.numel() * 4)
            outs.append(ff.to("cpu", non_blocking=True))
    side.synchronize()
    ctx.finish()
    for k, (z, ff) in enumerate(zip(seq, outs)):
        got = ff.numpy().reshape(H, W, 4)
        assert np.array_equal(got.view(np.uint32), twins[z].view(np.uint32)), (k, float(z))
    assert not np.array_equal(twins[zs[0]], twins[zs[2]])             # the planes do hide different records: a stale plane would be noticed
    ctx.set_stream(None)
    ctx.close()
    print("depth plane hand-off ok:", len(seq), "frames")


if __name__ == "__main__":
    main()
