"""Item dealing of the raster stage (tinycarlo_amd/csrc/tc_deal.h): the scan form -- one marker per entry that starts in
a pass's window, an inclusive max-scan over the 64 lanes, the carry from pass to pass -- hands every item to the entry the
literal binary search through the prefix table finds, at the same offset.  The header is built with the host compiler
(tests/deal_shim.py) and the 64 lanes are emulated; a third, independent answer comes from numpy (np.repeat)."""
import subprocess

import numpy as np
import pytest

import deal_shim


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return deal_shim.build_shim(tmp_path_factory.mktemp("tc_deal"))


def check(shim, cnt, n_tab=None):
    cnt = np.asarray(cnt, dtype=np.int32)
    want_owner = np.repeat(np.arange(len(cnt), dtype=np.int32), cnt)
    want_offset = (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)).astype(np.int32)
    so, sf, passes = deal_shim.deal(shim, cnt, n_tab, "scan")
    bo, bf, _ = deal_shim.deal(shim, cnt, n_tab, "search")
    assert np.array_equal(bo, want_owner) and np.array_equal(bf, want_offset), "the binary search itself"
    assert np.array_equal(so, bo), (cnt.tolist(), so.tolist(), bo.tolist())
    assert np.array_equal(sf, bf), (cnt.tolist(), sf.tolist(), bf.tolist())
    assert passes == (int(cnt.sum()) + 63) // 64
    return passes


def test_every_small_count_vector(shim):
    """every count vector of up to 6 entries with counts 0..5 (zeros at the head, in the middle and at the tail among them),
    as a table of its own size and padded to the kernels' 64 and 128 entries"""
    import ctypes as C
    nv = C.c_long(0)
    bad = shim.deal_exhaustive(6, 5, C.byref(nv))
    assert nv.value == sum(6 ** n for n in range(1, 7))  # none left out
    assert bad == 0


def test_small_vectors_against_numpy(shim):
    """a sample of the same family through the Python-side check (owner and offset against np.repeat)"""
    for cnt in ([0], [5], [0, 0, 3], [3, 0, 0], [0, 2, 0, 0, 4, 0], [1, 1, 1, 1, 1, 1], [5, 0, 5, 0, 5, 0], [0, 0, 0, 0, 0, 1]):
        check(shim, cnt)
        check(shim, cnt, 64)
        check(shim, cnt, 128)


@pytest.mark.parametrize("n", [64, 128])
def test_random_tables_of_several_passes(shim, n):
    """totals up to 1000: up to 16 passes, entries longer than a pass (a window no entry starts in: the carry alone) and runs
    of empty entries"""
    rng = np.random.default_rng(100 + n)
    seen_multi, seen_empty_window = 0, 0
    for rep in range(300):
        total = int(rng.integers(1, 1001))
        live = rng.choice(n, size=int(rng.integers(1, n + 1)), replace=False)
        cnt = np.bincount(rng.choice(live, size=total), minlength=n).astype(np.int32)
        passes = check(shim, cnt)
        seen_multi += passes > 1
        pre = np.cumsum(cnt) - cnt
        starts = np.unique(pre[cnt > 0] // 64)
        seen_empty_window += len(starts) < passes
    assert seen_multi > 100 and seen_empty_window > 10  # (the cases the test is about did occur)


@pytest.mark.parametrize("n", [64, 128])
def test_all_items_in_one_entry(shim, n):
    for at in (0, 1, n // 2, n - 1):
        for total in (1, 63, 64, 65, 128, 1000):
            cnt = np.zeros(n, np.int32)
            cnt[at] = total
            check(shim, cnt)


def test_exact_pass_boundaries(shim):
    """an entry that starts on the first and on the last slot of a window, and totals that are whole passes"""
    for cnt in ([64, 1], [63, 1, 64], [64, 64, 64], [1, 63, 1, 127, 1], [0, 64, 0, 64, 0]):
        check(shim, cnt, 64)


def test_standalone_program_under_sanitizers(tmp_path):
    exe = deal_shim.build_program(tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip().endswith("mismatches 0"), r.stdout
