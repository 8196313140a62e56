"""Parameters taken out into torch tensors, as a program of its own (tests/test_gpu_decompose.py starts it): torch must initialise its HIP runtime
BEFORE libgs4d.so is loaded into the process, which a pytest session that has already rendered frames cannot arrange.

tests/gpu_build_from_torch.py in the other direction.  For each form: the records are uploaded, transformed on the device and decomposed; every
destination is handed to a torch side stream (named with set_stream) through Context.read_tensor — gs4d_buffer_device_ptr, gs4d_buffer_invalidate,
then a device-to-device copy on that stream — and consumed there by a torch kernel, then the set is transformed and decomposed again into the same
destinations, with no host synchronisation anywhere in between.  Both sets of tensors must hold the rows of the host definition.  Exit code 0 = they do."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
torch.cuda.init()
import decompose_cases as dc      # noqa: E402

N = 1000


def main():
    side = torch.cuda.Stream()
    gs4d = importlib.import_module("4dgaussiansplatrendering_amd")
    rows_xf = [gs4d.affine4((0.8, 0.6, 0.0, 0.0), 1.5, (10.0, -20.0, 30.0)), gs4d.affine4((0.6, 0.0, 0.8, 0.0), 0.5, (-1.0, 2.0, -3.0), (0.25, 0.0, 0.5), 2.0, 1.0)]
    for which in ("3d", "4d_2q"):
        form, rows = dc.form_of(gs4d, which), dc.rows_of(gs4d, which)
        rec = dc.records(gs4d, which, N)
        ctx = gs4d.Context(64, 64)
        try:
            ctx.read_tensor(ctx.buffer(nbytes=64), torch.zeros(16, device="cuda"))
            raise AssertionError("read_tensor took a tensor whose stream was never named")
        except gs4d.Gs4dError:
            pass
        ctx.set_stream(side.cuda_stream)
        first, moved = ctx.buffer(rec), ctx.buffer(nbytes=96 * N)
        xf = [ctx.buffer(np.ascontiguousarray(r, np.float32).reshape(1, 20)) for r in rows_xf]
        bufs = {k: ctx.buffer(nbytes=4 * w * N) for k, w in rows.items()}
        outs = []
        with torch.cuda.stream(side):
            for step in range(2):
                ctx.transform_records(first, N, xf[step], 1, dst=moved)
                ctx.decompose_records(moved, N, form, **bufs)
                tensors = {k: torch.empty((N, w), dtype=torch.float32, device="cuda") for k, w in rows.items()}
                for k in rows:
                    ctx.read_tensor(bufs[k], tensors[k])
                outs.append({k: (t * 1.0).to("cpu", non_blocking=True) for k, t in tensors.items()})      # consumed on the caller's stream
        side.synchronize()
        ctx.finish()
        for step, got in enumerate(outs):
            want = gs4d.decompose_records_host(gs4d.transform_records_host(rec, rows_xf[step]), form)
            dc.assert_same({k: v.numpy() for k, v in got.items()}, want, f"{which}, step {step}")
        assert not np.array_equal(outs[0]["scale"].numpy(), outs[1]["scale"].numpy()), f"{which}: the second transform changed nothing: stale rows would go unnoticed"
        ctx.set_stream(None)
        ctx.close()
    print("decompose to torch ok: 2 forms")


if __name__ == "__main__":
    main()
