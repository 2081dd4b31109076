"""The stored-entry count of the set-up sweep (csrc/fused_sweep.hip, k_fz_cells<1, ...>) by itself.

The sweep shares no word between its workgroups: every workgroup leaves ONE count, by a plain store, in the scratch behind
nksr_fused_op_t.nnz_counter (op['nnz_scratch']: one word per workgroup, no initial value), and k_fz_count_sum adds the words into
the counter (op['nnz_counter'], one int64).  What can go wrong: a workgroup that does not write its word (`clumps`: a workgroup
without rows returns early), a word counted twice or left from the call before, a counter that is not reset by a second call,
a count that changes b or diag, and the call with no counter at all.  Every case fills the scratch and the operator's workspace
with 0xFF bytes first and runs the set-up twice; the count is compared with the non-zero slots of the integer rows of
tests/fused_op_ref.py (operator_ref), exactly."""
import numpy as np
import pytest
import torch

import fused_op_ref as fr
import test_gpu_fused_operator as tfo

pytestmark = pytest.mark.gpu

LAYOUTS = sorted(fr.LAYOUTS)
assert 'clumps' in LAYOUTS and 'segments2' in LAYOUTS


def _integer_operator(name):
    L, fld, op = tfo._operator(name)
    rc, nb = L['row_cells'], L['nbr']
    rows, t, xs = fr.integer_case(rc, nb, seed=7)
    fld.dense_rows(op).copy_(tfo._t(rows.astype(np.float32)))
    op['targets_all'].copy_(tfo._t(t.astype(np.float32)))
    ref = fr.operator_ref(rows, rc, nb, t, xs[0], 1.0)
    return fld, op, ref


def _poison(op):
    tfo._poison(op)
    op['nnz_scratch'].fill_(-1)         # 0xFF in every byte


def _bits(v):
    return v.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('name', LAYOUTS)
def test_count_equals_the_non_zero_slots_after_each_of_two_calls(name):
    from nksr_amd import _lib
    fld, op, ref = _integer_operator(name)
    assert op['nnz_counter'].shape == (1,) and op['nnz_counter'].dtype == torch.int64
    assert op['nnz_scratch'].numel() == (int(_lib.lib.nksr_fused_item_entries(op['rows_total'])) - 1) // 8      # one word per workgroup
    assert op['nnz_scratch'].numel() + 1 == int(_lib.lib.nksr_fused_count_words(op['rows_total']))
    out = []
    for call in range(2):
        _poison(op)
        b, diag = fld.fused_rhs_diag(op, 1.0)
        got = int(op['nnz_counter'].cpu().numpy()[0])
        print('%s call %d: counted %d, reference %d' % (name, call, got, ref['nnz']))
        assert got == ref['nnz'], '%s, call %d: counted %d stored entries, the rows hold %d' % (name, call, got, ref['nnz'])
        # every workgroup wrote its word (none keeps the fill), and the words add up to the total
        words = op['nnz_scratch'].cpu().numpy()
        assert (words >= 0).all() and int(words.sum()) == ref['nnz']
        out.append((_bits(b), _bits(diag)))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), name + ': b / diag differ between two calls'
    fr.compare_exact(name + ':b', out[0][0].view(np.float32), ref['b'])
    fr.compare_exact(name + ':diag', out[0][1].view(np.float32), ref['diag'])


def test_set_up_without_a_counter_gives_the_same_b_and_diag():
    fld, op, ref = _integer_operator('clumps')
    _poison(op)
    b, diag = fld.fused_rhs_diag(op, 1.0)
    assert int(op['nnz_counter'].cpu().numpy()[0]) == ref['nnz']
    counted = (_bits(b), _bits(diag))
    saved = op['op'].nnz_counter
    op['op'].nnz_counter = None
    try:
        _poison(op)
        op['nnz_counter'].fill_(-3)
        b, diag = fld.fused_rhs_diag(op, 1.0)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(b), counted[0]) and np.array_equal(_bits(diag), counted[1])
        # nothing of the count was touched
        assert int(op['nnz_counter'].cpu().numpy()[0]) == -3 and bool((op['nnz_scratch'] == -1).all())
    finally:
        op['op'].nnz_counter = saved
