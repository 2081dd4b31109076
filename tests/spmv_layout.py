"""numpy encoders of the streaming SpMV's two physical layouts (include/nksr_hip.h, col_format), for tests that build a CSR by hand:
a restatement of the layout in the tests' own words, independent of what nksr_assemble writes and of solver.csr_logical."""
import numpy as np

CHUNK = {0: 4096, 1: 4608}      # entries per chunk of the kernel = the unit the storage is zero-padded to


def encode0(cols, vals):
    """format 0: 256-entry tiles, entry m of a tile at 4 (m % 64) + m / 64, int32 columns; zero-padded to a multiple of 4096."""
    nnz = len(cols)
    k = np.arange(nnz)
    m = k & 255
    phys = (k & ~255) + 4 * (m & 63) + (m >> 6)
    npad = (nnz + 4095) // 4096 * 4096
    c, v = np.zeros(npad, np.int32), np.zeros(npad, np.float32)
    c[phys], v[phys] = cols, vals
    return c, v


def encode1(cols, vals):
    """format 1 before the packing: 192-entry tiles, entry m at 3 (m % 64) + m / 64; zero-padded to a multiple of 4608.  Returns
    int64 columns (three consecutive ones make a 64-bit word: pack21 here, nksr_pack_cols21 on the device) and the values."""
    nnz = len(cols)
    k = np.arange(nnz)
    t, m = k // 192, k % 192
    phys = t * 192 + 3 * (m & 63) + (m >> 6)
    npad = (nnz + 4607) // 4608 * 4608
    c, v = np.zeros(npad, np.int64), np.zeros(npad, np.float32)
    c[phys], v[phys] = cols, vals
    return c, v


def pack21(c):
    """three 21-bit columns per 64-bit word"""
    return c[0::3] | (c[1::3] << 21) | (c[2::3] << 42)
