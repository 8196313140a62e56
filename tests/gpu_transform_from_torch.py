"""Transforms that live in a torch tensor, as a program of its own (tests/test_gpu_transform.py starts it): torch must initialise its HIP runtime BEFORE
libgs4d.so is loaded into the process, which a pytest session that has already rendered frames cannot arrange.

A device tensor of gs4d_affine4 rows goes through Context.write_tensor into the xf buffer on a torch side stream (named with set_stream) and the set is
transformed; then the tensor is rewritten by a kernel on that stream, written again and the set transformed again into a second buffer, with no host
synchronisation anywhere in between.  Both results must be those of the host definition for the rows as they were at each call.  Exit code 0 = they are."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
torch.cuda.init()
import transform_cases as tc      # noqa: E402

N = 769


def main():
    side = torch.cuda.Stream()
    gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
    rows = tc.rows(("rigid", "scale_shear", "retime"))
    moved = rows * np.float32(0.5)                                  # what the kernel below makes of the tensor: exact in float32
    for which in ("4d_vel", "hostile"):
        rec = tc.records(gs4d, which, N)
        ctx = gs4d.Context(64, 64)
        ctx.set_stream(side.cuda_stream)
        src, xf = ctx.buffer(rec), ctx.buffer(nbytes=rows.nbytes)
        first, second = ctx.buffer(nbytes=96 * 3 * N), ctx.buffer(nbytes=96 * 3 * N)
        with torch.cuda.stream(side):
            tensor = torch.from_numpy(rows).to("cuda")
            ctx.write_tensor(xf, tensor)
            ctx.transform_records(src, N, xf, 3, dst=first)
            tensor.mul_(0.5)                                        # rewritten on the side stream, by a kernel the host does not wait for
            ctx.write_tensor(xf, tensor)                            # ... into the buffer the first call may still be reading
            ctx.transform_records(src, N, xf, 3, dst=second)
        side.synchronize()
        ctx.finish()
        for what, buf, r in (("first", first, rows), ("rewritten", second, moved)):
            got = ctx.read(buf, np.float32, 3 * N * 24).reshape(3 * N, 24)
            ok = tc.same_bits(got, tc.expected(gs4d, rec, r))
            assert ok.all(), f"{which}, {what}: {int((~ok).any(1).sum())} records differ from the host definition"
        assert not tc.same_bits(tc.expected(gs4d, rec, rows), tc.expected(gs4d, rec, moved)).all()
        ctx.set_stream(None)
        ctx.close()
    print("transform from torch ok")


if __name__ == "__main__":
    main()
