"""The device sample buffer (tinycarlo_amd.SampleBuffer, tc_collect) against its definition (tinycarlo_amd.collect.
collect_reference, plain numpy): every array and every counter for equality.

Synthetic calls without an env (tests/collect_cases.py: N over wavefront and workgroup borders, frames of 4 / 20 / 2560 /
12288 bytes for both access paths, the three overflow modes, strides, next_obs, columns of 1 / 4 / 8 bytes, three calls of
12 / 5 / 1 rows in rotating order, destinations pre-filled with 0xFF; tests/test_collect_cpu.py asserts on the reference alone
that each case has re-spawn rows inside calls and across borders, skipped steps, overflow and same-call clashes), a captured
call replayed twice, and simple_layout end to end through drive().  Run on the MI355X box with `pytest -m gpu`."""
import copy
import os

import numpy as np
import pytest

import collect_cases as cc
from common import load_cfg
from tinycarlo_amd import collect as col
from tinycarlo_amd.packing import unpack_bits_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TORCH_COLUMNS = {"flag": torch.uint8, "maneuver": torch.int32, "steer": torch.float64}
CASES = cc.gpu_cases()


def make_buffer(case, max_rows=12):
    from tinycarlo_amd import SampleBuffer
    buf = SampleBuffer(case.capacity, case.N, (case.F,), columns=TORCH_COLUMNS, next_obs=case.next_obs, stride=case.stride,
                       overflow=case.overflow, seed=case.seed, max_rows=max_rows, device=DEV)
    for t in [buf.obs, buf.next_obs, buf.env] + list(buf.cols.values()):  # every destination starts as 0xFF bytes
        if t is not None:
            t.view(torch.uint8).fill_(0xFF)
    buf.begin(torch.from_numpy(case.begin_obs).to(DEV), torch.from_numpy(case.begin_pending).to(DEV))
    return buf


def to_dev(rows):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in rows.items()}


def assert_equals_reference(buf, st, what):
    torch.cuda.synchronize()
    for k in ("obs", "next_obs", "ordinal", "env", "pending", "age", "last"):
        t = getattr(buf, k)
        if st[k] is None:
            assert t is None, (what, k)
            continue
        got = t.cpu().numpy()
        if not np.array_equal(got, st[k]):
            bad = np.nonzero((got != st[k]).reshape(len(got), -1).any(1))[0]
            raise AssertionError((what, k, "first differing rows", bad[:8].tolist(), "of", len(bad)))
    for k, t in buf.cols.items():
        assert np.array_equal(t.cpu().numpy().view(np.uint8), st["cols"][k].view(np.uint8)), (what, "column", k)
    c = buf.counters.cpu().numpy()
    assert (int(c[0]), int(c[1]), int(c[2])) == (st["count"], st["next_ordinal"], st["dropped"]), (what, c.tolist())
    assert len(buf) == st["count"] and buf.dropped == st["dropped"] and buf.full == (st["count"] >= len(st["ordinal"]))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_synthetic_calls_equal_the_definition(case):
    buf = make_buffer(case)
    st = case.new_state()
    for c, rows in enumerate(case.calls):
        before = st["next_ordinal"]
        col.collect_reference(st, rows, case.stride, case.overflow, case.seed)
        buf.collect(to_dev(rows))
        assert_equals_reference(buf, st, (case.id, "call", c))
        assert int(buf.counters[3]) == st["next_ordinal"] - before
    assert st["next_ordinal"] > 0


def test_misaligned_frames_take_the_four_byte_path():
    """F = 2560 is a multiple of 16, but rows that start 4 bytes into an allocation are not 16-byte aligned: same results"""
    case = cc.Case(301, 70, 2560, (5, 12, 1), cc.SMALL, "ring", 1, True)
    buf = make_buffer(case)
    st = case.new_state()
    for c, rows in enumerate(case.calls):
        col.collect_reference(st, rows, case.stride, case.overflow, case.seed)
        d = to_dev(rows)
        raw = torch.empty(d["obs"].numel() + 16, dtype=torch.uint8, device=DEV)
        shifted = raw[4:4 + d["obs"].numel()].view(d["obs"].shape)
        shifted.copy_(d["obs"])
        assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
        buf.collect({**d, "obs": shifted})
        assert_equals_reference(buf, st, ("shifted", c))


def test_rows_without_done_flags_and_columns_passed_apart():
    case = cc.Case(302, 63, 20, (5, 1, 12), cc.BIG, "stop", 2, False)
    buf = make_buffer(case)
    st = case.new_state()
    for c, rows in enumerate(case.calls):
        plain = {k: v for k, v in rows.items() if k not in ("terminated", "truncated")}
        col.collect_reference(st, plain, case.stride, case.overflow, case.seed)
        d = to_dev(plain)
        buf.collect({"obs": d["obs"]}, columns={k: d[k] for k in cc.COLUMNS})
        assert_equals_reference(buf, st, ("no flags", c))
    with pytest.raises(ValueError):
        buf.collect({"obs": torch.zeros((13, case.N, case.F), dtype=torch.uint8, device=DEV)}, columns={})  # K > max_rows
    with pytest.raises(ValueError):
        buf.collect({"obs": to_dev(case.calls[0])["obs"]})  # a column is missing


@pytest.mark.parametrize("overflow", cc.MODES)
def test_captured_collect_replayed_twice(overflow):
    case = cc.Case(303, 70, 2560, (12, 5, 1), cc.SMALL, overflow, 2, True)
    buf = make_buffer(case)
    rows = to_dev(case.calls[0])
    make_buffer(case).collect(rows)  # (a first launch outside the capture, on a buffer of its own: loads the kernels)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # one linear stream
        with torch.cuda.graph(g, stream=s):
            buf.collect(rows)
    torch.cuda.synchronize()
    st = case.new_state()
    assert_equals_reference(buf, st, "capture alone changes nothing")
    for r in range(2):
        g.replay()
        col.collect_reference(st, case.calls[0], case.stride, case.overflow, case.seed)
        assert_equals_reference(buf, st, ("replay", r))
    assert st["next_ordinal"] > case.capacity


def test_state_dict_round_trip_and_sample_index():
    case = cc.Case(304, 70, 20, (12, 5, 1), cc.SMALL, "random", 1, True)
    a, b = make_buffer(case), make_buffer(case)
    calls = [to_dev(r) for r in case.calls]
    a.collect(calls[0])
    b.load_state_dict(a.state_dict())
    for r in calls[1:]:
        a.collect(r)
        b.collect(r)
    assert_equals_reference(a, case.reference(), "a")
    assert_equals_reference(b, case.reference(), "restored")
    half = make_buffer(cc.Case(305, 70, 20, (1,), cc.SMALL, "stop", 1, False))
    idx = half.sample_index(64)
    assert idx.dtype == torch.int64 and idx.tolist() == [0] * 64  # (empty: zeros, nothing out of range)
    half.collect(to_dev(half_case_rows()))
    n = len(half)
    assert 0 < n < cc.SMALL
    gen = torch.Generator(device=DEV).manual_seed(1)
    idx = half.sample_index(4096, generator=gen)
    assert int(idx.min()) == 0 and int(idx.max()) == n - 1  # (4096 draws over fewer than 97 slots reach both ends)
    s = half.sample(idx[:8], torch.uint8)
    assert np.array_equal(s["obs"].cpu().numpy(), half.obs.cpu().numpy()[idx[:8].cpu().numpy()])
    assert np.array_equal(s["steer"].cpu().numpy(), half.cols["steer"].cpu().numpy()[idx[:8].cpu().numpy()])


def half_case_rows():
    return cc.Case(305, 70, 20, (1,), cc.SMALL, "stop", 1, False).calls[0]


# ------------------------------------------------------------------ end to end on simple_layout
N_ENVS, LIMIT, CALLS = 70, 5, (12, 12, 1)


def cfg_for():
    cfg, path = load_cfg("simple_layout")
    cfg = copy.deepcopy(cfg)
    cfg["camera"]["resolution"] = [64, 64]
    cfg["sim"]["observation_space_format"] = "classes"
    cfg["map"]["json_path"] = os.path.join(os.path.dirname(path), cfg["map"]["json_path"])
    return cfg


@pytest.mark.parametrize("packing", ("bits", None), ids=("packed", "byte"))
def test_end_to_end_on_simple_layout(packing):
    from tinycarlo_amd.vec_env import TinyCarloVecEnv
    vec = TinyCarloVecEnv(cfg_for(), num_envs=N_ENVS, device=DEV, autoreset=True, spawn="device", obs_packing=packing)
    vec.set_time_limit(LIMIT)
    obs0, _ = vec.reset(seed=3)
    vec.episode_stats["length"].copy_((torch.arange(N_ENVS, device=DEV) * LIMIT // N_ENVS).to(torch.int32))  # staggered
    vec.set_controller(k=4.0, speed=0.4)
    vec.randomize_drive(maneuvers=(0, 1, 3), mode="cycle", ou=dict(theta=0.1, mu=0.0, sigma=0.4, reset=False), seed=9)
    with pytest.raises(ValueError):
        vec.make_sample_buffer(64, columns=("camera",))       # no camera bank installed
    with pytest.raises(ValueError):
        vec.make_sample_buffer(64, columns=("laneline_distances",))  # not [K, N]
    stride, cap = 2, 150
    buf = vec.make_sample_buffer(cap, columns=("maneuver", "steer"), stride=stride, overflow="ring", next_obs=True, max_rows=12)
    assert buf.packed == (packing == "bits") and buf.obs_shape == tuple(vec.out["obs"].shape[1:])
    assert buf.cols["maneuver"].dtype == torch.int32 and buf.cols["steer"].dtype == torch.float64
    buf.begin(vec.out["obs"])
    st = col.reference_state(cap, N_ENVS, buf.obs_shape, {"maneuver": np.int32, "steer": np.float64}, next_obs=True)
    col.reference_begin(st, vec.out["obs"].cpu().numpy())
    keys = ("obs", "reward", "terminated", "truncated", "maneuver", "steer")
    respawn_inside = pending_border = skipped = 0
    for c, K in enumerate(CALLS):
        roll = vec.alloc_rollout(K, keys=keys)
        vec.drive(None, roll)
        before = {k: v.clone() for k, v in roll.items()}
        buf.collect(roll)
        torch.cuda.synchronize()
        for k in keys:  # the env's rollouts are untouched by a collect
            assert torch.equal(before[k], roll[k]), k
        host = {k: v.cpu().numpy() for k, v in roll.items()}
        # non-vacuity, on the rollouts themselves
        done = (host["terminated"] | host["truncated"]) != 0
        pend, age = st["pending"].astype(bool).copy(), st["age"].copy()
        pending_border += int(pend.sum())
        for k in range(K):
            respawn_inside += int(pend.sum()) if k > 0 else 0
            act = ~pend
            skipped += int((act & (age % stride != 0)).sum())
            age = np.where(pend, 0, age + 1)
            pend = done[k]
        col.collect_reference(st, host, stride, "ring", 0)
        assert np.array_equal(st["age"], age)
        assert_equals_reference(buf, st, (packing, "call", c))
    assert respawn_inside > 0 and pending_border > 0 and skipped > 0
    assert st["next_ordinal"] > cap and st["count"] == cap  # slots were overwritten
    assert len(set(st["cols"]["maneuver"].tolist())) > 1 and st["obs"].any()
    idx = torch.tensor([0, cap - 1, 7, 7, 33], dtype=torch.int64, device=DEV)
    for dtype in (torch.float32, torch.uint8):
        s = buf.sample(idx, dtype)
        for name in ("obs", "next_obs"):
            frames = st[name][idx.cpu().numpy()]
            if packing == "bits":
                want = unpack_bits_reference(frames, 64, dtype)
            else:
                want = torch.from_numpy(frames) if dtype == torch.uint8 else torch.from_numpy(frames).to(dtype) / 255
            assert tuple(s[name].shape) == (5, vec.n_classes, 64, 64) and s[name].dtype == dtype
            assert torch.equal(s[name].cpu(), want), (packing, name, dtype)
        assert np.array_equal(s["maneuver"].cpu().numpy(), st["cols"]["maneuver"][idx.cpu().numpy()])
        assert np.array_equal(s["steer"].cpu().numpy().view(np.int64), st["cols"]["steer"][idx.cpu().numpy()].view(np.int64))
        assert np.array_equal(s["env"].cpu().numpy(), st["env"][idx.cpu().numpy()])
    vec.close()
