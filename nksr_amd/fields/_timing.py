"""NKSR_TIMING_DETAIL=1: synchronised sub-stage times of the solve set-up, one table for every module of the split
(fields/kernel_field.py re-exports DETAIL_TIMES: bench.py reads it there)."""
import os
import time

import torch

_DETAIL = os.environ.get('NKSR_TIMING_DETAIL', '') == '1'
DETAIL_TIMES = {}


def _tick(name, t0):
    """Time since ``t0`` accumulated under ``name`` in DETAIL_TIMES (diagnostics only); returns the new start."""
    if not _DETAIL:
        return t0
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    DETAIL_TIMES[name] = DETAIL_TIMES.get(name, 0.0) + (t1 - t0)
    return t1
