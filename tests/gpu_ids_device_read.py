"""gs4d_read_ids_device into torch tensors, as a program of its own: torch must initialise its HIP runtime BEFORE libgs4d.so is loaded
into the process (tests/gpu_aux_device_read.py has the same constraint).  Exit code 0 = the tensors equal gs4d_read_ids bit for bit."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
torch.cuda.init()
import scenes                     # noqa: E402

gs4d = importlib.import_module("4dgaussiansplatrendering_amd")


def main():
    n, W, H = 20000, 640, 360
    pos, q, scale, rgba = scenes.cube_params(n, seed=4)
    rec = gs4d.build_records_3d(pos, q, scale * 3.0, rgba)
    cam = scenes.CAM_CUBE
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.set_id_outputs(True)
    db, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
    ctx.clear()
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
    ctx.keygen(db, 0.0, cam[0], kb, ib, n)
    ctx.sort_pairs(kb, ib, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)
    planes = [torch.full((H, W), 7, dtype=torch.int32, device="cuda") for _ in range(3)]
    only_w = torch.full((H, W), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()      # the fills run on torch's stream, which the library's reads are not ordered after (no gs4d_set_stream here)
    ctx.read_ids_device(planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(), W * H * 4)
    ctx.read_ids_device(None, None, only_w.data_ptr(), W * H * 4)            # one plane alone
    ctx.finish()
    want = ctx.read_ids()
    ctx.close()
    got = [p.cpu().numpy().view(np.uint32) for p in planes]
    ok = all(np.array_equal(g, w.view(np.uint32)) for g, w in zip(got, want)) and np.array_equal(only_w.cpu().numpy().view(np.uint32), want[2].view(np.uint32))
    if not ok or (want[0] != 0xFFFFFFFF).mean() <= 0.05:
        print("ids device read differs", [int((g != w.view(np.uint32)).sum()) for g, w in zip(got, want)], int((only_w.cpu().numpy().view(np.uint32) != want[2].view(np.uint32)).sum()), float((want[0] != 0xFFFFFFFF).mean()))
        return 1
    print("ids device read ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
