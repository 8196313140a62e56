"""Parameters that live in torch tensors, as a program of its own (tests/test_gpu_build.py starts it): torch must initialise its HIP runtime BEFORE
libgs4d.so is loaded into the process, which a pytest session that has already rendered frames cannot arrange.

For each form: device tensors go through Context.write_tensor into the parameter buffers on a torch side stream (named with set_stream), the records
are built on the device and drawn, and the frame is read back on the device and consumed on the same stream — then the tensors are rewritten by
kernels on that stream, written again, built and drawn again, with no host synchronisation anywhere in between.  Both pictures must have the bits of
the host route's: the host builders' records uploaded into a fresh context.  Exit code 0 = they do."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
torch.cuda.init()
import build_cases as bc          # noqa: E402
import scenes                     # noqa: E402

W, H, N = 64, 48, 300
CAM, CAM_DIR = (0.0, 0.0, 150.0), (0.0, 0.0, -1.0)


def frame(gs4d, ctx, db, kb, ib, n, t):
    ctx.clear()
    ctx.keygen(db, t, CAM, kb, ib, n)
    ctx.sort_pairs(kb, ib, n)
    ctx.bind(1, ib)
    ctx.bind(2, db)
    ctx.draw_instanced(n)


def new_context(gs4d, t):
    ctx = gs4d.Context(W, H)
    ctx.set_clear_color(gs4d.CLEAR_COLOR)
    ctx.set_mode(gs4d.MODE_4D_SORTED)
    ctx.set_uniforms(time=t, min_opacity=0.0, view=gs4d.look_at(CAM, CAM_DIR), proj=gs4d.perspective(scenes.FOV, W, H, scenes.ZNEAR, scenes.ZFAR))
    return ctx


def host_route(gs4d, form, p, t):
    ctx = new_context(gs4d, t)
    db, kb, ib = ctx.buffer(bc.host_records(gs4d, form, p)), ctx.buffer(nbytes=4 * N), ctx.buffer(nbytes=4 * N)
    frame(gs4d, ctx, db, kb, ib, N, t)
    img = ctx.read_pixels()
    ctx.close()
    return img


def main():
    side = torch.cuda.Stream()
    gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
    for form in bc.FORMS:
        t = bc.picture_time(form)
        p = bc.picture_set(gs4d, form, N)
        moved = dict(p, pos=p["pos"].copy(), scale=p["scale"] * np.float32(2.0))       # what the kernels below make of the tensors: exact in float32
        moved["pos"][:, :3] *= np.float32(0.5)
        ctx = new_context(gs4d, t)
        try:
            ctx.write_tensor(ctx.buffer(nbytes=64), torch.zeros(16, device="cuda"))
            raise AssertionError("write_tensor took a tensor whose stream was never named")
        except gs4d.Gs4dError:
            pass
        ctx.set_stream(side.cuda_stream)
        bufs = {k: ctx.buffer(nbytes=a.nbytes) for k, a in p.items()}
        db, kb, ib = ctx.buffer(nbytes=96 * N), ctx.buffer(nbytes=4 * N), ctx.buffer(nbytes=4 * N)
        outs = []
        with torch.cuda.stream(side):
            tensors = {k: torch.from_numpy(a).to("cuda") for k, a in p.items()}
            for step in range(2):
                if step == 1:                                      # rewritten on the side stream, by kernels the host does not wait for
                    tensors["pos"][:, :3].mul_(0.5)
                    tensors["scale"].mul_(2.0)
                for k in p:
                    ctx.write_tensor(bufs[k], tensors[k])
                assert ctx.build_records(bc.form_id(gs4d, form), N, dst=db, **bufs) == db
                frame(gs4d, ctx, db, kb, ib, N, t)
                ff = torch.empty(H * W * 4, dtype=torch.float32, device="cuda")
                ctx.read_pixels_device(ff.data_ptr(), ff.numel() * 4)
                outs.append(ff.to("cpu", non_blocking=True))       # consumed on the caller's stream
        side.synchronize()
        ctx.finish()
        assert ctx.shadow_builds(db) == 2
        clear = np.array(gs4d.CLEAR_COLOR, np.float32)
        for what, got, params in (("first", outs[0], p), ("rewritten", outs[1], moved)):
            got, want = got.numpy().reshape(H, W, 4), host_route(gs4d, form, params, t)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{form}, {what}: {int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum())} pixels differ from the host route"
            assert int((np.abs(got - clear).max(-1) > 1.0 / 255.0).sum()) > 100, f"{form}, {what}: an empty frame"
        assert not np.array_equal(outs[0].numpy(), outs[1].numpy()), f"{form}: the rewritten tensors changed nothing: stale parameters would go unnoticed"
        ctx.set_stream(None)
        ctx.close()
    print("build from torch ok:", len(bc.FORMS), "forms")


if __name__ == "__main__":
    main()
