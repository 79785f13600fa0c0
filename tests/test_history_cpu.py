"""Frame histories of the sample buffer without a GPU: the definition with links (tinycarlo_amd.collect.collect_reference /
history_reference) against the history-less run and against a trace of the links worked out apart from it, the rules of
tinycarlo_amd/csrc/tc_collect.h (built alone by the host compiler, tests/history_shim.py; once more as a stand-alone program
under -fsanitize=address,undefined) against the definition, the non-vacuity of the cases the GPU tests use
(tests/history_cases.py), the header / binding, and the argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import collect_cases as cc
import history_cases as hc
import history_shim
from common import ROOT
from tinycarlo_amd import collect as col

CASES = cc.gpu_cases()
DEDICATED = hc.dedicated_cases()
ALL = DEDICATED + CASES


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return history_shim.build_shim(tmp_path_factory.mktemp("tc_history"))


PLAIN_KEYS = ("obs", "next_obs", "ordinal", "env", "pending", "age", "last")


def assert_same_plain(a, b, what):
    """every array and counter of a history-less state"""
    for k in PLAIN_KEYS:
        if a[k] is None:
            assert b[k] is None, (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)
    assert a["cols"].keys() == b["cols"].keys()
    for k in a["cols"]:
        assert np.array_equal(a["cols"][k].view(np.uint8), b["cols"][k].view(np.uint8)), (what, "column", k)
    for k in ("count", "next_ordinal", "dropped"):
        assert int(a[k]) == int(b[k]), (what, k)


# ------------------------------------------------------------------ the definition
def test_reference_state_gains_links_only_when_asked():
    plain = col.reference_state(8, 3, (4,), {"a": np.int32}, True)
    assert "prev" not in plain and "chain" not in plain
    st = col.reference_state(8, 3, (4,), {"a": np.int32}, True, history=True)
    assert set(st) == set(plain) | {"prev", "chain"}
    assert st["prev"].dtype == st["chain"].dtype == np.int64 and (st["prev"] == -1).all() and (st["chain"] == -1).all()
    assert st["prev"].shape == (8,) and st["chain"].shape == (3,)
    st["chain"][:] = 5
    col.reference_begin(st, np.zeros((3, 4), dtype=np.uint8))
    assert (st["chain"] == -1).all()
    with pytest.raises(ValueError):
        col.history_reference(plain, [0], 2)
    for kw in (dict(T=0), dict(T=2, pad="wrap"), dict(T=2, overflow="fifo")):
        with pytest.raises(ValueError):
            col.history_reference(st, [0], **kw)


@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_links_change_nothing_else_and_equal_the_trace(case):
    plain = case.new_state()
    for c, rows in enumerate(case.calls):
        col.collect_reference(plain, rows, case.stride, case.overflow, case.seed)
        assert_same_plain(plain, hc.reference(case, c + 1), (case.id, "call", c))
    st = hc.reference(case)
    prev, chain = hc.link_trace(case)
    assert np.array_equal(st["prev"], prev), case.id
    assert np.array_equal(st["chain"], chain), case.id
    # a link is an earlier ordinal of the same env; a slot nothing was written to has none
    assert (st["prev"][st["ordinal"] < 0] == -1).all() and (st["prev"] < st["ordinal"])[st["ordinal"] >= 0].all()


def test_history_frames_follow_the_slots():
    """obs[b, t] is the frame of slots[b, t] (zeros for -1), next_obs is the queue shifted by one, edge repeats the last"""
    case = DEDICATED[0]
    st = hc.reference(case)
    index = hc.sample_index(st)
    zero = col.history_reference(st, index, 4, "zero", case.overflow, case.seed)
    edge = col.history_reference(st, index, 4, "edge", case.overflow, case.seed)
    assert zero["slots"].shape == (len(index), 4) and zero["valid"].dtype == np.int32 and zero["obs"].shape == (len(index), 4, case.F)
    assert np.array_equal(zero["valid"], edge["valid"]) and (zero["valid"][-2:] == 0).all() and (zero["slots"][-2:] == -1).all()
    for b in range(len(index)):
        v = int(zero["valid"][b])
        assert (zero["slots"][b, v:] == -1).all() and np.array_equal(zero["slots"][b, :v], edge["slots"][b, :v])
        assert (edge["slots"][b, v:] == (edge["slots"][b, v - 1] if v else -1)).all()
        for t in range(4):
            s = zero["slots"][b, t]
            assert np.array_equal(zero["obs"][b, t], st["obs"][s] if s >= 0 else np.zeros(case.F, dtype=np.uint8))
        if v:
            assert np.array_equal(zero["next_obs"][b, 0], st["next_obs"][index[b]])
            # stride 1: the frame after a step is the frame before the env's next step
            for t in range(1, v):
                assert np.array_equal(st["next_obs"][zero["slots"][b, t]], st["obs"][zero["slots"][b, t - 1]])
        assert np.array_equal(zero["next_obs"][b, 1:], zero["obs"][b, :-1])
        assert np.array_equal(edge["next_obs"][b, 1:], edge["obs"][b, :-1])
    one = col.history_reference(st, index, 1, "zero", case.overflow, case.seed)
    assert np.array_equal(one["slots"][:, 0], np.where(one["valid"] > 0, index, -1))


# ------------------------------------------------------------------ tc_collect.h against the definition
@pytest.mark.parametrize("case", ALL, ids=[c.id for c in ALL])
def test_header_rules_equal_the_definition(shim, case):
    mine = hc.new_state(case)
    for c, rows in enumerate(case.calls):
        link = history_shim.run_call(shim, mine, rows, case.stride, case.overflow, case.seed)
        ref = hc.reference(case, c + 1)
        assert_same_plain(ref, mine, (case.id, "call", c))
        assert np.array_equal(ref["prev"], mine["prev"]) and np.array_equal(ref["chain"], mine["chain"]), (case.id, "call", c)
        assert (link >= -1).all()  # (every entry of link_rows is written)
    ref = hc.reference(case)
    index = hc.sample_index(ref)
    for T in hc.TS:
        for pad in hc.PADS:
            want = col.history_reference(ref, index, T, pad, case.overflow, case.seed)
            slots, valid = history_shim.run_history(shim, mine, index, T, pad, case.overflow, case.seed)
            assert np.array_equal(slots, want["slots"]) and np.array_equal(valid, want["valid"]), (case.id, T, pad)


def test_sanitized_program_runs_every_mode(tmp_path):
    """the link rule and the resolve walk as a stand-alone program (its own main) under -fsanitize=address,undefined, built
    once and run once over one file per mode with the definition's results beside the inputs"""
    exe = history_shim.build_program(tmp_path)
    cases = DEDICATED[:2] + [c for c in CASES if c.overflow == "stop" and c.capacity == cc.SMALL and c.N == 70][:1]
    assert {c.overflow for c in cases} == set(cc.MODES)
    files = []
    for case in cases:
        st = hc.reference(case)
        files.append(str(tmp_path / f"{case.overflow}.bin"))
        with open(files[-1], "wb") as f:
            f.write(history_shim.program_input(case, st, hc.sample_index(st), hc.TS))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(ln.endswith("wrong 0") for ln in lines), r.stdout
    bad = tmp_path / "bad.bin"   # a wrong expectation is noticed
    data = bytearray(open(files[0], "rb").read())
    data[-1] ^= 1
    bad.write_bytes(bytes(data))
    assert subprocess.run([exe, str(bad)], capture_output=True, text=True, timeout=120).returncode == 1


# ------------------------------------------------------------------ the shared cases test something
@pytest.mark.parametrize("case", DEDICATED, ids=[c.id for c in DEDICATED])
def test_dedicated_cases_have_all_four_kinds(case):
    st = hc.reference(case)
    for T in (2, 4):
        n = hc.categories(case, st, T)
        print(case.id, T, n)
        assert n["full"] > 0 and n["start"] > 0 and n["lost"] > 0 and n["crossing"] > 0, (case.id, T, n)
        assert n["full"] + n["start"] + n["lost"] == n["samples"] == case.capacity
    assert hc.categories(case, st, 19)["full"] == 0  # 18 rows: no chain is that long


def test_the_worked_example_of_the_rules():
    case = DEDICATED[0]
    assert case.id == "N70-F20-K12_5_1-cap400-ring-s1-x1"
    assert hc.categories(case, hc.reference(case), 4) == dict(full=80, start=192, lost=128, crossing=136, samples=400)


def test_existing_cases_in_sum_and_stop_mode():
    total = dict(full=0, start=0, lost=0, crossing=0, samples=0)
    stop_big = 0
    for case in CASES:
        st = hc.reference(case)
        n = hc.categories(case, st, 4)
        for k, v in n.items():
            total[k] += v
        assert hc.categories(case, st, 19)["full"] == 0, case.id
        if case.overflow == "stop":
            assert n["lost"] == 0, (case.id, n)  # stop mode overwrites nothing, and a dropped ordinal has no later slot
            if case.capacity == cc.BIG and case.N > 1:
                stop_big += 1
                assert n["full"] > 0 and n["start"] > 0 and n["crossing"] > 0, (case.id, n)
    print(total)
    assert stop_big >= 4
    assert (total["full"], total["start"], total["lost"], total["samples"]) == (11341, 19699, 754, 31794)
    assert total["crossing"] > 0


# ------------------------------------------------------------------ header and binding
def test_header_declares_and_binding_lists_the_entry_points(shim):
    from tinycarlo_amd import _native as nat
    h = open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()
    assert re.search(r"#define TC_HAS_HISTORY 1\b", h) and nat.HAS_HISTORY == 1
    assert re.search(r"#define TC_ABI_VERSION 7\b", h) and nat.ABI_VERSION == 7
    for name, v in col.PAD.items():
        assert re.search(r"#define TC_PAD_%s %d\b" % (name.upper(), v), h)
    L = nat.lib()
    assert L.tc_abi_version() == 7
    for name in ("tc_collect_link", "tc_history_resolve", "tc_gather_frames"):
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in nat.EXPORTS and hasattr(L, name), name
    assert C.sizeof(col.CollectDescC) == 8 + 4 * 4 + 8 + 8 + 4 * 8 + 8 * 24 + 6 * 8  # tc_collect_desc is as it was
    for rows, n in ((1, 1), (12, 70), (128, 4096), (5, 64), (5, 65)):
        want = 16 + rows * ((n + 63) // 64) * 8 + (rows * ((n + 63) // 64) * 4 + 15) // 16 * 16
        assert L.tc_collect_scratch_bytes(rows, n) == shim.shim_scratch_size(rows, n) == want
    assert L.tc_collect_scratch_bytes(0, 5) == 0 and L.tc_collect_scratch_bytes(5, 0) == 0


def test_new_kernels_keep_out_of_the_kernel_name_pattern():
    """tests/test_variant_matrix_cpu.py lists every tc_*_kernel symbol; the history kernels are named as the collect kernels"""
    src = "".join(open(os.path.join(ROOT, "tinycarlo_amd", "csrc", f)).read() for f in ("k_collect.h", "k_history.h"))
    names = re.findall(r"void (tc_\w+)\(", src)
    assert {"tc_collect_link_scan", "tc_collect_link_rank", "tc_collect_link_walk", "tc_history_resolve_walk", "tc_gather_frames_k"} <= set(names)
    assert not [n for n in names if n.endswith("_kernel")]


# ------------------------------------------------------------------ argument checks, each before any HIP call
def test_invalid_arguments_return_before_any_hip_call():
    """the pointers below are host memory and are never dereferenced: every call returns TC_E_INVALID with a text on a
    machine without a device (the valid forms are not called here: they would reach the device)"""
    from tinycarlo_amd import _native as nat
    L = nat.lib()
    mem = np.zeros(1 << 16, dtype=np.uint8)
    base = mem.ctypes.data + (-mem.ctypes.data) % 16

    def at(i, off=0):  # distinct 16-byte aligned host addresses (+ off)
        return base + 4096 * i + off

    def link(desc_over=None, n_rows=3, null_desc=False, chain=at(5), rows=at(6)):
        d = col.CollectDescC()
        d.capacity, d.num_envs, d.stride, d.mode, d.n_columns, d.frame_bytes = 16, 5, 1, 0, 0, 32
        d.pending, d.age, d.counters, d.scratch, d.scratch_bytes = at(0), at(1), at(2), at(3), 4096
        for k, v in (desc_over or {}).items():
            setattr(d, k, v)
        return L.tc_collect_link(None if null_desc else C.byref(d), n_rows, at(4), at(4), chain, rows, None)
    bad = [dict(null_desc=True), dict(n_rows=0), dict(chain=None), dict(rows=None), dict(chain=at(5, 4)), dict(rows=at(6, 4)),
           dict(n_rows=2 ** 15, desc_over={"num_envs": 2 ** 11, "scratch_bytes": 2 ** 40})]
    bad += [dict(desc_over=o) for o in ({"pending": None}, {"age": None}, {"counters": None}, {"scratch": None}, {"capacity": 0},
                                        {"num_envs": 0}, {"stride": 0}, {"age": at(1, 2)}, {"counters": at(2, 4)}, {"scratch": at(3, 8)},
                                        {"scratch_bytes": L.tc_collect_scratch_bytes(3, 5) - 1})]
    for kw in bad:
        assert link(**kw) == -1, kw
        assert b"tc_collect_link" in L.tc_last_error(), kw

    def resolve(**over):
        a = dict(prev=at(0), ordinal=at(1), capacity=16, mode=1, seed=0, index=at(2), n_index=4, T=3, pad=0, slots=at(3),
                 next_slots=at(4), valid=at(5))
        a.update(over)
        return L.tc_history_resolve(a["prev"], a["ordinal"], a["capacity"], a["mode"], a["seed"], a["index"], a["n_index"], a["T"], a["pad"],
                                    a["slots"], a["next_slots"], a["valid"], None)
    for over in (dict(prev=None), dict(ordinal=None), dict(index=None), dict(slots=None), dict(valid=None), dict(capacity=0), dict(T=0),
                 dict(n_index=-1), dict(mode=3), dict(mode=-1), dict(pad=2), dict(pad=-1), dict(mode=2, capacity=2 ** 32),
                 dict(prev=at(0, 4)), dict(ordinal=at(1, 4)), dict(index=at(2, 4)), dict(slots=at(3, 4)), dict(next_slots=at(4, 4)),
                 dict(valid=at(5, 2))):
        assert resolve(**over) == -1, over
        assert b"tc_history_resolve" in L.tc_last_error(), over
    assert resolve(n_index=0) == 0  # nothing to do: no launch

    def gather(**over):
        a = dict(src=at(0), src2=None, n_src=4, F=32, index=at(2), n_out=4, group=1, dst=at(3), dtype=nat.F16)
        a.update(over)
        return L.tc_gather_frames(a["src"], a["src2"], a["n_src"], a["F"], a["index"], a["n_out"], a["group"], a["dst"], a["dtype"], None)
    for over in (dict(src=None), dict(index=None), dict(dst=None), dict(n_src=0), dict(F=0), dict(F=30), dict(n_out=-1),
                 dict(src2=at(1), group=0), dict(dtype=nat.F64), dict(dtype=9), dict(src=at(0, 2)), dict(src2=at(1, 1)),
                 dict(index=at(2, 4)), dict(dst=at(3, 8))):
        assert gather(**over) == -1, over
        assert b"tc_gather_frames" in L.tc_last_error(), over
    assert gather(n_out=0) == 0


def test_sample_buffer_argument_checks_need_no_device():
    import torch
    from tinycarlo_amd import SampleBuffer
    ok = dict(capacity=8, num_envs=4, obs_shape=(2, 4, 4))
    for over in (dict(history=0), dict(history=-2), dict(history=2, next_obs=True, stride=2),
                 dict(history=2, columns={str(i): torch.int32 for i in range(8)})):
        with pytest.raises(ValueError):
            SampleBuffer(**{**ok, **over})
    # what must pass these checks fails only at the device, which a CPU tensor device is not
    for over in (dict(history=2, next_obs=True, stride=1), dict(history=2, stride=2), dict(history=1, next_obs=True, stride=2),
                 dict(history=3, columns={str(i): torch.int32 for i in range(7)}), dict(columns={str(i): torch.int32 for i in range(8)})):
        with pytest.raises(ValueError, match="lives on the GPU"):
            SampleBuffer(**{**ok, **over, "device": "cpu"})


class _NoLinks:
    """a SampleBuffer's attributes as sample() reads them before it touches a tensor"""
    history, prev = 1, None


def test_sample_argument_checks_need_no_device():
    from tinycarlo_amd import SampleBuffer
    with pytest.raises(ValueError, match="no links"):
        SampleBuffer.sample(_NoLinks(), None, history=2)
    with pytest.raises(ValueError, match="pad"):
        SampleBuffer.sample(_NoLinks(), None, pad="wrap")
    with pytest.raises(ValueError, match="at least 1"):
        SampleBuffer.sample(_NoLinks(), None, history=0)
