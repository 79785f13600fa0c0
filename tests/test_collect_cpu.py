"""The sample buffer without a GPU: the definition (tinycarlo_amd.collect.collect_reference) against a transcription of the
loop it restates, the rules of tinycarlo_amd/csrc/tc_collect.h (built alone by the host compiler, tests/collect_shim.py) against
the definition, the counter-based replacement draw, the header / binding, the argument checks of tc_collect, and the
non-vacuity of the synthetic cases the GPU tests use (tests/collect_cases.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import collect_cases as cc
import collect_shim
from common import ROOT
from tinycarlo_amd import collect as col
from tinycarlo_amd.randomization import draw_replace_slot


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return collect_shim.build_shim(tmp_path_factory.mktemp("tc_collect"))


def assert_same_state(a, b, what):
    for k in ("obs", "next_obs", "ordinal", "env", "pending", "age", "last"):
        if a[k] is None:
            assert b[k] is None, (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)
    assert a["cols"].keys() == b["cols"].keys()
    for k in a["cols"]:
        assert np.array_equal(a["cols"][k].view(np.uint8), b["cols"][k].view(np.uint8)), (what, "column", k)
    for k in ("count", "next_ordinal", "dropped"):
        assert int(a[k]) == int(b[k]), (what, k, a[k], b[k])


# ------------------------------------------------------------------ the definition against the script's loop
def script_loop(env_rows, first_obs, first_pending, skip_steps):
    """examples/train_stanley_il.py:59-77 over ONE env's row stream, episode after episode: `obs` is what reset() or the
    previous step returned, the sample of action step i (counted from the episode's reset) pairs it with that step's
    command, `i % SKIP_STEPS == 0` keeps it, and the episode ends behind a terminated | truncated step.  A batched env's
    stream has one extra row per episode end, the re-spawn row, which is the next episode's reset(): its frame is that
    reset's obs (the synthetic rows may flag a re-spawn row too: rule 3 then makes the next row a re-spawn row again).  -> list of (obs, next_obs, maneuver, steer)"""
    X = []
    t, T = 0, len(env_rows)
    obs = first_obs
    def reset():                # obs, info = env.reset(): the re-spawn row (one that is flagged itself is followed by another)
        nonlocal t
        while t < T:
            row = env_rows[t]
            t += 1
            if not (row["terminated"] or row["truncated"]):
                return row["obs"], True
        return None, False
    more = True
    if first_pending:           # the stream opens with a re-spawn row
        obs, more = reset()
    while more and t < T:       # sample_episode
        i = 0
        while t < T:
            row = env_rows[t]   # env.step(action)
            t += 1
            if i % skip_steps == 0:
                X.append((obs, row["obs"], row["maneuver"], row["steer"]))
            obs = row["obs"]
            i += 1
            if row["terminated"] or row["truncated"]:
                break
        else:
            break               # the stream ends inside an episode
        obs, more = reset()
    return X


@pytest.mark.parametrize("stride", (1, 2, 3))
def test_definition_equals_the_scripts_loop_per_env(stride):
    case = cc.Case(7, 9, 20, (12, 5, 1, 12), cc.BIG, "stop", stride, True)
    st = case.reference()
    assert st["dropped"] == 0 and st["count"] == st["next_ordinal"] > 0
    seen = 0
    for n in range(case.N):
        stream = [{k: rows[k][kk, n] for k in ("obs", "terminated", "truncated", "maneuver", "steer")}
                  for rows in case.calls for kk in range(rows["obs"].shape[0])]
        want = script_loop(stream, case.begin_obs[n], bool(case.begin_pending[n]), stride)
        mine = np.nonzero(st["env"][:st["count"]] == n)[0]  # (stop mode below capacity: slots in ordinal order)
        assert len(mine) == len(want), (n, len(mine), len(want))
        for slot, (o, o1, m, y) in zip(mine, want):
            assert np.array_equal(st["obs"][slot], o) and np.array_equal(st["next_obs"][slot], o1), (n, slot)
            assert st["cols"]["maneuver"][slot] == m and st["cols"]["steer"][slot] == y, (n, slot)
        seen += len(want)
    assert seen == st["count"]
    if stride > 1:
        assert seen < sum(case.Ks) * case.N * 0.8


def test_rows_without_done_flags_have_no_respawn_row():
    case = cc.Case(3, 5, 4, (4, 3), cc.BIG, "stop", 1, False)
    st = col.reference_state(cc.BIG, 5, (4,), {"maneuver": np.int32})
    col.reference_begin(st, case.begin_obs)
    for rows in case.calls:
        col.collect_reference(st, {"obs": rows["obs"], "maneuver": rows["maneuver"]})
    assert st["count"] == 7 * 5 and not st["pending"].any() and (st["age"] == 7).all()
    assert np.array_equal(st["obs"][:5], case.begin_obs) and np.array_equal(st["obs"][5:10], case.calls[0]["obs"][0])


# ------------------------------------------------------------------ tc_collect.h against the definition
@pytest.mark.parametrize("overflow", cc.MODES)
@pytest.mark.parametrize("stride,next_obs,capacity", [(1, True, cc.SMALL), (2, False, cc.SMALL), (3, True, 31), (1, False, cc.BIG)])
def test_header_rules_equal_the_definition(shim, overflow, stride, next_obs, capacity):
    case = cc.Case(11, 70, 20, (12, 5, 1, 12, 12), capacity, overflow, stride, next_obs)
    ref, mine = case.new_state(), case.new_state()
    for c, rows in enumerate(case.calls):
        before = ref["next_ordinal"]
        col.collect_reference(ref, rows, stride, overflow, case.seed)
        n_cand = collect_shim.run_call(shim, mine, rows, stride, overflow, case.seed)
        assert n_cand == ref["next_ordinal"] - before
        assert_same_state(ref, mine, (overflow, "call", c))
    if capacity != cc.BIG:
        assert ref["next_ordinal"] > capacity and (ref["dropped"] > 0) == (overflow == "stop")


def test_draw_replace_slot_equals_the_header(shim):
    rng = np.random.default_rng(0)
    for cap in (1, 2, 97, 25000, 2 ** 32 - 1):
        o = np.concatenate([np.arange(cap, cap + 50, dtype=np.int64), rng.integers(0, 2 ** 62, 50)])
        for seed in (0, 5, 2 ** 64 - 1):
            got = draw_replace_slot(seed, o, cap)
            assert got.dtype == np.int64 and (got >= 0).all() and (got < cap).all()
            assert [int(v) for v in got] == [shim.shim_replace_slot(seed, int(v), cap) for v in o]
    many = draw_replace_slot(3, np.arange(97, 97 + 97 * 200), 97)
    assert abs(np.bincount(many, minlength=97) - 200).max() < 80  # (uniform: 200 +- a few sigma of 14 per slot)
    with pytest.raises(ValueError):
        draw_replace_slot(0, 5, 2 ** 32)


def test_sanitized_program_runs_every_mode(tmp_path):
    """tc_collect.h and the shim as a stand-alone program (its own main) under -fsanitize=address,undefined, built once and
    run once over one file per mode with the definition's results beside the inputs"""
    exe = collect_shim.build_program(tmp_path)
    files = []
    for overflow in cc.MODES:
        case = cc.Case(13, 70, 20, (12, 1, 5), cc.SMALL, overflow, 2, True)
        files.append(str(tmp_path / f"{overflow}.bin"))
        with open(files[-1], "wb") as f:
            f.write(collect_shim.program_input(case))
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3 and all(ln.endswith("wrong 0") for ln in lines), r.stdout


# ------------------------------------------------------------------ header and binding
def test_header_declares_and_binding_lists_the_entry_points():
    from tinycarlo_amd import _native as nat
    h = open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()
    assert "int tc_collect(" in h and "int64_t tc_collect_scratch_bytes(" in h
    assert "tc_collect" in nat.EXPORTS and "tc_collect_scratch_bytes" in nat.EXPORTS
    assert re.search(r"#define TC_ABI_VERSION 7\b", h) and nat.ABI_VERSION == 7
    assert re.search(r"#define TC_HAS_COLLECT 1\b", h) and nat.HAS_COLLECT == 1
    for name, v in col.OVERFLOW.items():
        assert re.search(r"#define TC_COLLECT_%s %d\b" % (name.upper(), v), h)
    assert re.search(r"#define TC_COLLECT_MAX_COLUMNS %d\b" % col.MAX_COLUMNS, h)
    L = nat.lib()
    assert L.tc_abi_version() == 7
    assert C.sizeof(col.CollectDescC) == 8 + 4 * 4 + 8 + 8 + 4 * 8 + 8 * 24 + 6 * 8


def test_scratch_bytes(shim):
    from tinycarlo_amd import _native as nat
    L = nat.lib()
    for rows, n in ((1, 1), (12, 70), (128, 4096), (5, 64), (5, 65)):
        want = 16 + rows * ((n + 63) // 64) * 8 + (rows * ((n + 63) // 64) * 4 + 15) // 16 * 16
        assert L.tc_collect_scratch_bytes(rows, n) == shim.shim_scratch_size(rows, n) == want
    assert L.tc_collect_scratch_bytes(0, 5) == 0 and L.tc_collect_scratch_bytes(5, 0) == 0


def test_invalid_arguments_return_before_any_hip_call():
    """every check of tc_collect comes before its first HIP call: the pointers below are host memory and are never
    dereferenced, and the call returns TC_E_INVALID with a text on a machine without a device"""
    from tinycarlo_amd import _native as nat
    L = nat.lib()
    K, N, F, cap = 3, 5, 32, 16
    mem = {k: np.zeros(n + 16, dtype=np.uint8) for k, n in dict(obs_rows=K * N * F, obs=cap * F, next_obs=cap * F, ordinal=cap * 8,
                                                                env=cap * 4, pending=N, age=N * 4, last=N * F, counters=32, scratch=4096,
                                                                src=K * N * 8, dst=cap * 8, done=K * N).items()}

    def at(k, off=0):  # a 16-byte aligned host address (+ off)
        p = mem[k].ctypes.data
        return p + (-p) % 16 + off

    def call(desc_over=None, n_rows=K, obs_rows="ok", null_desc=False, **cols):
        d = col.CollectDescC()
        d.capacity, d.num_envs, d.stride, d.mode, d.n_columns, d.seed, d.frame_bytes = cap, N, 1, 0, 1, 0, F
        for k in ("obs", "next_obs", "ordinal", "env", "pending", "age", "last", "counters", "scratch"):
            setattr(d, k, at(k))
        d.scratch_bytes = 4096
        d.columns[0].src, d.columns[0].dst, d.columns[0].elem_size = at("src"), at("dst"), 8
        for k, v in (desc_over or {}).items():
            setattr(d, k, v)
        for k, v in cols.items():
            setattr(d.columns[0], k, v)
        rows = at("obs_rows") if obs_rows == "ok" else obs_rows
        return L.tc_collect(None if null_desc else C.byref(d), n_rows, rows, at("done"), at("done"), None)

    bad = [dict(null_desc=True), dict(obs_rows=None), dict(n_rows=0), dict(n_rows=-1), dict(obs_rows=at("obs_rows", 2)),
           dict(src=None), dict(dst=None), dict(elem_size=2), dict(elem_size=0), dict(src=at("src", 4)), dict(dst=at("dst", 1))]
    bad += [dict(desc_over={k: None}) for k in ("obs", "ordinal", "env", "pending", "age", "last", "counters", "scratch")]
    bad += [dict(desc_over=o) for o in (
        {"capacity": 0}, {"num_envs": 0}, {"num_envs": -3}, {"frame_bytes": 0}, {"frame_bytes": 30}, {"stride": 0}, {"mode": 3}, {"mode": -1},
        {"n_columns": 9}, {"n_columns": -1}, {"mode": 2, "capacity": 2 ** 32}, {"obs": at("obs", 1)}, {"next_obs": at("next_obs", 2)},
        {"last": at("last", 3)}, {"ordinal": at("ordinal", 4)}, {"counters": at("counters", 4)}, {"env": at("env", 2)}, {"age": at("age", 1)},
        {"scratch": at("scratch", 8)}, {"scratch_bytes": 16}, {"scratch_bytes": L.tc_collect_scratch_bytes(K, N) - 1},
        {"num_envs": 2 ** 30})]
    # (one wavefront per (row, env) in the copy launch: 2^26 pairs would be a grid of 2^32 threads)
    bad.append(dict(n_rows=2 ** 15, desc_over={"num_envs": 2 ** 11, "scratch_bytes": 2 ** 40}))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"tc_collect" in L.tc_last_error(), kw
    # (the valid form is not called here: it would reach the device)


def test_sample_buffer_argument_checks_need_no_device():
    import torch
    from tinycarlo_amd import SampleBuffer
    ok = dict(capacity=8, num_envs=4, obs_shape=(2, 4, 4))
    for over in (dict(overflow="fifo"), dict(capacity=0), dict(stride=0), dict(obs_shape=(3, 3)), dict(columns={"a": torch.float16}),
                 dict(columns={"obs": torch.int32}), dict(columns={str(i): torch.int32 for i in range(9)}), dict(max_rows=0),
                 dict(device="cpu")):
        with pytest.raises(ValueError):
            SampleBuffer(**{**ok, **over})


# ------------------------------------------------------------------ the shared cases test something
def test_gpu_cases_are_not_vacuous():
    cases = cc.gpu_cases()
    assert len({c.id for c in cases}) == len(cases) == 48
    assert {c.N for c in cases} == set(cc.NS) and {c.F for c in cases} == set(cc.FS)
    assert {(c.N, c.F, c.overflow) for c in cases} == {(n, f, m) for n in cc.NS for f in cc.FS for m in cc.MODES}
    assert {(c.overflow, c.capacity, c.stride, c.next_obs) for c in cases} == set(cc._COMBOS)
    big_ring = 0
    for c in cases:
        assert sorted(c.Ks) == [1, 5, 12]
        _, s = c.trace()
        st = c.reference()
        assert s["respawn_inside"] > 0 and s["pending_border"] > 0, (c.id, s)
        if c.stride > 1:
            assert s["skipped"] > 0, (c.id, s)
        if cc.can_overflow(c):
            if c.overflow == "stop":
                assert s["dropped"] > 0 and st["dropped"] == s["dropped"], (c.id, s)
            else:
                assert s["overwritten"] > 0 and st["dropped"] == 0, (c.id, s)
            if c.overflow == "random":
                assert s["same_call_clash"] > 0, (c.id, s)
            big_ring += c.overflow == "ring" and s["max_call"] > c.capacity
        else:
            assert st["next_ordinal"] <= c.capacity and st["count"] == st["next_ordinal"], c.id
        assert st["next_ordinal"] == sum(len(x) for x in c.trace()[0])
    assert big_ring >= 1  # a ring call with more candidates than the capacity
    for m in cc.MODES:
        assert sum(cc.can_overflow(c) and c.overflow == m for c in cases) >= 4, m
