"""The order hint's launch-order table on x86 (csrc/dcol_device.hpp hint_fill_window_scalar,
hint_entry_index, hint_window_len; tests/hint_table): the table of a 3-window launch whose
last window is ragged, built from given hint bytes under a non-identity perm, against the
rule stated independently here -- the stable descending sort of the clamped bytes inside each
window, position p of window v at entry ((p // ppw) * wins + v) * ppw + p % ppw."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hint_table")
_i32, _i64, _P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
_SIGNATURES = {
    "hint_table_windows": (_i32, [_i64, _i32, _i32]),
    "hint_table_window_len": (_i32, [_i64, _i64, _i32]),
    "hint_table_entry_index": (_i64, [_i64, _i32, _i32, _i32]),
    "hint_table_solve_blocks": (_i64, [_i32, _i32]),
    "hint_table_build": (_i32, [_i64, _i64, _i64, _i32, _i32, _P, _P, _P, _P, _P, _i64]),
}


@pytest.fixture(scope="module")
def lib():
    subprocess.run(["make", "-C", DIR, "-s"], check=True)
    L = ctypes.CDLL(os.path.join(DIR, "libhint_table.so"))
    for name, (res, args) in _SIGNATURES.items():
        getattr(L, name).restype, getattr(L, name).argtypes = res, args
    return L


LENGTHS = (1, 31, 32, 33, 127, 128, 129, 255, 256)
PPW = (64, 32, 16, 8)   # pairs per wave at 1, 2, 4, 8 lanes per pair
WW = (1, 4, 8)
SLOT0 = 37              # the launch is a bucket in the middle of a plan
GUARD = 24              # entries before and after the launch's share of the table
FILL = -99


def _byte_arrays(n, rng):
    yield "random", rng.integers(0, 256, n)
    yield "counts", rng.integers(4, 13, n)      # what a run leaves: a few distinct counts
    yield "equal", np.full(n, 7)
    yield "clamped", rng.integers(60, 70, n)    # around the clamp at 63


def _launch(length, ppw, ww):
    """slots of a launch of three windows whose last one holds `length` slots (folded into 1 .. ws)"""
    ws = ww * ppw
    return 2 * ws + (length - 1) % ws + 1, ws


@pytest.mark.parametrize("ww", WW)
@pytest.mark.parametrize("ppw", PPW)
@pytest.mark.parametrize("length", LENGTHS)
def test_table_of_a_ragged_three_window_launch(lib, length, ppw, ww):
    n, ws = _launch(length, ppw, ww)
    lpp = 64 // ppw
    B = SLOT0 + n + 11
    rng = np.random.default_rng(1000 * length + 10 * ppw + ww)
    perm = rng.permutation(B).astype(np.int32)
    s1 = rng.integers(0, 1000, B).astype(np.int32)
    s2 = rng.integers(0, 1000, B).astype(np.int32)
    wins = lib.hint_table_windows(n, lpp, ww)
    assert wins == 8 and wins * ws >= n                     # 3 windows padded to a multiple of 8
    assert lib.hint_table_solve_blocks(wins, ww) == wins * ww
    lens = [lib.hint_table_window_len(n, v, ws) for v in range(wins)]
    assert lens == [ws, ws, n - 2 * ws] + [0] * 5
    entries = wins * ww * ppw
    for name, hb in _byte_arrays(B, rng):
        h = np.ascontiguousarray(hb, np.uint8)
        tab = np.full((GUARD + entries + GUARD, 4), FILL, np.int32)
        got = lib.hint_table_build(B, SLOT0, n, lpp, ww, h.ctypes.data, perm.ctypes.data, s1.ctypes.data,
                                   s2.ctypes.data, tab.ctypes.data, GUARD)
        assert got == wins
        assert np.all(tab[:GUARD] == FILL) and np.all(tab[GUARD + entries:] == FILL), name
        t = tab[GUARD:GUARD + entries]
        assert not np.any(t == FILL), name                  # every entry of the launch is written
        # the entries with a pair are exactly the launch's slots, each once
        live = t[:, 0] >= 0
        assert sorted(t[live, 3].tolist()) == list(range(n)), name
        want = np.full((entries, 4), -1, np.int32)
        key = np.minimum(h.astype(np.int64), 63)
        for v in range(3):
            slots = np.arange(v * ws, v * ws + lens[v])
            order = slots[np.argsort(-key[SLOT0 + slots], kind="stable")]
            if name == "equal":
                np.testing.assert_array_equal(order, slots)
            for p, slot in enumerate(order):
                e = ((p // ppw) * wins + v) * ppw + p % ppw   # wave rank * wins + v, lane group p % ppw
                assert e == lib.hint_table_entry_index(v, p, ppw, wins)
                pi = perm[SLOT0 + slot]
                want[e] = (pi, s1[pi], s2[pi], slot)
        # every slot at its place with its perm / s1 / s2; phantom and ragged entries all -1
        np.testing.assert_array_equal(t, want, err_msg=name)
        if name == "equal":   # the identity: wave rank * wins + v, group g solves slot v * ws + rank * ppw + g
            w, g = np.divmod(np.arange(entries), ppw)
            slot = (w % wins) * ws + (w // wins) * ppw + g
            np.testing.assert_array_equal(t[:, 3], np.where(slot < n, slot, -1))


def test_identity_perm_is_the_slot(lib):
    n, ws = _launch(33, 32, 4)
    B = n
    s = np.arange(B, dtype=np.int32)
    h = np.zeros(B, np.uint8)
    wins = lib.hint_table_windows(n, 2, 4)
    tab = np.full((wins * 4 * 32, 4), FILL, np.int32)
    r = s[::-1].copy()
    lib.hint_table_build(B, 0, n, 2, 4, h.ctypes.data, None, s.ctypes.data, r.ctypes.data, tab.ctypes.data, 0)
    live = tab[tab[:, 0] >= 0]
    np.testing.assert_array_equal(live[:, 0], live[:, 3])          # no perm: the pair is the slot
    np.testing.assert_array_equal(live[:, 1], live[:, 0])
    np.testing.assert_array_equal(live[:, 2], B - 1 - live[:, 0])
