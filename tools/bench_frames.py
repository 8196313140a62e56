#!/usr/bin/env python3
"""Frames a bench.py run rendered on its measured context, from its JSON line: the warm-up steps it ran (warmup_steps_run) plus
--steps x --windows per timed-window attempt.  With several lines (one file each) they must agree; prints the count.
usage: bench_frames.py <line file> [<line file> ...]"""
import json
import sys


def frames(path):
    lines = [ln for ln in open(path).read().splitlines() if ln.startswith("{")]
    d = json.loads(lines[-1])
    return d["warmup_steps_run"] + d["steps"] * len(d["windows_ms_per_step"]) * d["timed_window_attempts"]


if __name__ == "__main__":
    counts = {frames(p) for p in sys.argv[1:]}
    if len(counts) != 1:
        sys.exit(f"bench_frames.py: the runs rendered different numbers of frames: {sorted(counts)}")
    print(counts.pop())
