"""gs4d_read_aux_device into a torch tensor, as a program of its own: torch must initialise its HIP runtime BEFORE libgs4d.so is loaded
into the process (tests/gpu_stream_handoff.py has the same constraint).  Exit code 0 = the tensor equals gs4d_read_aux bit for bit."""
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
    ctx.set_aux_outputs(True)
    db, kb, ib = ctx.buffer(rec), ctx.buffer(nbytes=4 * n), ctx.buffer(nbytes=4 * n)
    ctx.clear()
    ctx.set_uniforms(time=0.0, min_opacity=0.0, view=gs4d.look_at(cam[0], cam[1]), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
    ctx.keygen(db, 0.0, cam[0], kb, ib, n)
    ctx.sort_pairs(kb, ib, n)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)
    t = torch.full((H, W, 2), -1.0, dtype=torch.float32, device="cuda")
    ctx.read_aux_device(t.data_ptr(), t.numel() * 4)
    ctx.finish()
    want = ctx.read_aux()
    ctx.close()
    got = t.cpu().numpy()
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)) or want[..., 1].max() <= 0.3:
        print("aux device read differs", float(np.abs(got - want).max()), float(want[..., 1].max()))
        return 1
    print("aux device read ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
