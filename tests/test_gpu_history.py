"""Frame histories of the device sample buffer (SampleBuffer(history=T): tc_collect_link, tc_history_resolve,
tc_gather_frames) against their definition (tinycarlo_amd.collect.collect_reference / history_reference, plain numpy):
everything for equality, no tolerance anywhere.

The synthetic cases are tests/history_cases.py's dedicated ones plus the 48 of tests/collect_cases.py (N over wavefront and
workgroup borders, frames of 4 / 20 bytes and 2560 / 12288 bytes for both access paths of the gather); tests/test_history_cpu.py
asserts on the reference alone that they hold full, start-cut and lost-predecessor histories and links across call borders.
A buffer with a history and next frames needs stride 1, so a case with stride 2 runs here without next frames (the numpy
definition of such a case, next frames included, is covered on the CPU).  Frames are compared on the device: the
definition's uint8 frames are uploaded once per (T, pad) and converted there with torch's `.to(dtype) / 255`.
Run on the MI355X box with `pytest -m gpu`."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import collect_cases as cc
import history_cases as hc
from common import load_cfg
from tinycarlo_amd import collect as col
from tinycarlo_amd.packing import unpack_bits_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
TORCH_COLUMNS = {"flag": torch.uint8, "maneuver": torch.int32, "steer": torch.float64}
DTYPES = (torch.uint8, torch.float16, torch.bfloat16, torch.float32)
GPU_TS = (1, 2, 4, 19)
CASES = hc.dedicated_cases() + cc.gpu_cases()
CHUNK_BYTES = 96 << 20  # uint8 bytes of one compared batch of histories


def device_case(case):
    """the case as a buffer with links can run it: next frames only at stride 1"""
    if case.next_obs and case.stride > 1:
        return cc.Case(case.seed, case.N, case.F, case.Ks, case.capacity, case.overflow, case.stride, False)
    return case


def make_buffer(case, history=4, max_rows=12, obs_shape=None, packed=False):
    from tinycarlo_amd import SampleBuffer
    shape = tuple(obs_shape) if obs_shape else (case.F,)
    buf = SampleBuffer(case.capacity, case.N, shape, columns=TORCH_COLUMNS, next_obs=case.next_obs, stride=case.stride,
                       overflow=case.overflow, seed=case.seed, max_rows=max_rows, device=DEV, packed=packed, history=history)
    for t in [buf.obs, buf.next_obs, buf.env] + list(buf.cols.values()):  # every destination starts as 0xFF bytes
        if t is not None:
            t.view(torch.uint8).fill_(0xFF)
    buf.begin(torch.from_numpy(case.begin_obs).to(DEV).view((case.N,) + shape), torch.from_numpy(case.begin_pending).to(DEV))
    return buf


def to_dev(rows, obs_shape=None):
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in rows.items()}
    if obs_shape:
        out["obs"] = out["obs"].view(tuple(out["obs"].shape[:2]) + tuple(obs_shape))
    return out


def assert_equals_reference(buf, st, what):
    """every array and counter the history-less test compares, then the links"""
    torch.cuda.synchronize()
    for k in ("obs", "next_obs", "ordinal", "env", "pending", "age", "last", "prev", "chain"):
        t = getattr(buf, k)
        if st[k] is None:
            assert t is None, (what, k)
            continue
        got = t.cpu().numpy().reshape(st[k].shape)
        if not np.array_equal(got, st[k]):
            bad = np.nonzero((got != st[k]).reshape(len(got), -1).any(1))[0]
            raise AssertionError((what, k, "first differing rows", bad[:8].tolist(), "of", len(bad)))
    for k, t in buf.cols.items():
        assert np.array_equal(t.cpu().numpy().view(np.uint8), st["cols"][k].view(np.uint8)), (what, "column", k)
    c = buf.counters.cpu().numpy()
    assert (int(c[0]), int(c[1]), int(c[2])) == (st["count"], st["next_ordinal"], st["dropped"]), (what, c.tolist())


def expected(frames_u8, dtype):
    """torch's own conversion of byte frames, on the device"""
    return frames_u8 if dtype == torch.uint8 else frames_u8.to(dtype) / 255


def assert_samples_equal_reference(buf, st, index, overflow, seed, Ts=GPU_TS, dtypes=DTYPES, what="", unpack_w=None):
    """sample(index, dtype, history=T, pad) against history_reference for every T, pad and dtype; unpack_w: the frames are
    packed rows of that many pixels and go through unpack_bits_reference"""
    F = int(np.prod(st["obs"].shape[1:]))
    for T in Ts:
        per = max(1, CHUNK_BYTES // (T * F))
        for pad in hc.PADS:
            for lo in range(0, len(index), per):
                part = np.ascontiguousarray(index[lo:lo + per])
                B = len(part)
                want = col.history_reference(st, part, T, pad, overflow, seed)
                idx = torch.from_numpy(part).to(DEV)
                names = ["obs"] + (["next_obs"] if want["next_obs"] is not None else [])
                if unpack_w is None:
                    dev_want = {k: torch.from_numpy(want[k]).to(DEV).reshape(B, T, F) for k in names}
                for dtype in dtypes:
                    s = buf.sample(idx, dtype, history=T, pad=pad)
                    tag = (what, "T", T, pad, dtype, "from", lo)
                    assert s["slots"].dtype == torch.int64 and tuple(s["slots"].shape) == (B, T) and s["valid"].dtype == torch.int32
                    assert np.array_equal(s["slots"].cpu().numpy(), want["slots"]), tag
                    assert np.array_equal(s["valid"].cpu().numpy(), want["valid"]), tag
                    for k in names:
                        got = s[k]
                        assert got.dtype == dtype and got.shape[0] == B and (T == 1 or got.shape[1] == T), tag
                        assert got.dim() == (1 if T == 1 else 2) + len(buf.obs_shape), tag
                        if unpack_w is None:
                            same = torch.equal(got.reshape(B, T, F), expected(dev_want[k], dtype))
                        else:
                            ref = unpack_bits_reference(want[k].reshape((B, T) + buf.obs_shape), unpack_w, dtype)
                            same = torch.equal(got.cpu().reshape(ref.shape), ref)
                        assert same, tag + (k,)
                # columns, env and ordinal: [B], of the newest entry
                ok = want["valid"] > 0
                newest = want["slots"][:, 0]
                assert np.array_equal(s["ordinal"].cpu().numpy(), np.where(ok, st["ordinal"][np.clip(newest, 0, None)], -1))
                assert np.array_equal(s["env"].cpu().numpy()[ok], st["env"][newest[ok]])
                for name, c in st["cols"].items():
                    assert tuple(s[name].shape) == (B,)
                    assert np.array_equal(s[name].cpu().numpy()[ok].view(np.uint8), c[newest[ok]].view(np.uint8)), (tag, name)


# ------------------------------------------------------------------ the device against the definition
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_synthetic_calls_and_samples_equal_the_definition(case):
    case = device_case(case)
    buf = make_buffer(case)
    for c in range(len(case.Ks)):
        buf.collect(to_dev(case.calls[c]))
        assert_equals_reference(buf, hc.reference(case, c + 1), (case.id, "call", c))
    st = hc.reference(case)
    assert st["next_ordinal"] > 0
    assert_samples_equal_reference(buf, st, hc.sample_index(st), case.overflow, case.seed, what=case.id)


def test_a_buffer_without_history_is_as_it_was():
    case = cc.Case(306, 70, 20, (12, 5, 1), cc.SMALL, "ring", 1, True)
    from tinycarlo_amd import SampleBuffer
    buf = SampleBuffer(case.capacity, case.N, (case.F,), columns=TORCH_COLUMNS, next_obs=True, overflow="ring", seed=case.seed, max_rows=12, device=DEV)
    assert buf.history == 1 and buf.prev is None and buf.chain is None and buf._link_rows is None and buf._desc.n_columns == 3
    buf.begin(torch.from_numpy(case.begin_obs).to(DEV), torch.from_numpy(case.begin_pending).to(DEV))
    buf.collect(to_dev(case.calls[0]))
    idx = torch.tensor([0, 5, 5, 96], dtype=torch.int64, device=DEV)
    s = buf.sample(idx, torch.float16)
    assert set(s) == {"obs", "next_obs", "env", "ordinal", "flag", "maneuver", "steer"} and tuple(s["obs"].shape) == (4, case.F)
    assert torch.equal(s["obs"], buf.obs[idx].to(torch.float16) / 255)
    assert set(buf.state_dict()) == {"obs", "next_obs", "ordinal", "env", "counters", "pending", "age", "last", "cols", "config"}
    assert "history" not in buf.state_dict()["config"]
    with pytest.raises(ValueError):
        buf.sample(idx, torch.float16, history=2)
    linked = make_buffer(case, history=2)
    with pytest.raises(ValueError):
        linked.load_state_dict(buf.state_dict())
    with pytest.raises(ValueError):
        buf.load_state_dict(linked.state_dict())
    empty = linked.sample(torch.empty(0, dtype=torch.int64, device=DEV), torch.float16)  # an empty batch launches nothing
    assert tuple(empty["obs"].shape) == (0, 2, case.F) and tuple(empty["slots"].shape) == (0, 2) and tuple(empty["valid"].shape) == (0,)


# ------------------------------------------------------------------ the gather kernel alone
def gather(src, src2, index, group, dtype, frame_shape):
    from tinycarlo_amd import _native as nat
    code = {torch.uint8: nat.U8, torch.float16: nat.F16, torch.bfloat16: nat.BF16, torch.float32: nat.F32}[dtype]
    F = int(np.prod(frame_shape))
    out = torch.empty((len(index),) + tuple(frame_shape), dtype=dtype, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    nat.check(nat.lib().tc_gather_frames(src.data_ptr(), src2.data_ptr() if src2 is not None else None, src.shape[0], F, index.data_ptr(),
                                         len(index), group, out.data_ptr(), code, stream), "tc_gather_frames")
    return out


@pytest.mark.parametrize("F", (256, 260), ids=("wide", "four_byte"))
def test_byte_conversion_is_torchs(F):
    """one frame with all 256 byte values in each float dtype: bit-equal to frames.to(dtype) / 255 computed by torch on the device"""
    frames = (torch.arange(2 * F, device=DEV) % 256).to(torch.uint8).view(2, F)
    assert len(set(frames[0].tolist())) == 256
    index = torch.tensor([0, 1, 0], dtype=torch.int64, device=DEV)
    for dtype in DTYPES:
        got = gather(frames, None, index, 1, dtype, (F,))
        want = expected(frames[index], dtype)
        assert got.dtype == want.dtype and torch.equal(got.view(torch.uint8), want.contiguous().view(torch.uint8)), dtype


@pytest.mark.parametrize("F", (2560, 12288, 20))
def test_misaligned_sources_take_the_four_byte_path(F):
    """source rows 4 bytes off a 16-byte boundary, a second source for every third output frame, indices outside the source"""
    n_src, rng = 9, np.random.default_rng(F)
    def shifted():
        raw = torch.empty(n_src * F + 16, dtype=torch.uint8, device=DEV)
        t = raw[4:4 + n_src * F].view(n_src, F)
        t.copy_(torch.from_numpy(rng.integers(0, 256, (n_src, F), dtype=np.uint8)))
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    a, b = shifted(), shifted()
    index = torch.tensor([3, -1, 8, 0, n_src, 5, 5, 2 ** 40, 1, -2 ** 40, 7], dtype=torch.int64, device=DEV)
    inside = ((index >= 0) & (index < n_src)).view(-1, 1)
    safe = index.clamp(0, n_src - 1)
    from_b = (torch.arange(len(index), device=DEV) % 3 == 0).view(-1, 1)
    want_u8 = torch.where(inside, torch.where(from_b, b[safe], a[safe]), torch.zeros((), dtype=torch.uint8, device=DEV))
    aligned_a, aligned_b = a.clone(), b.clone()
    assert aligned_a.data_ptr() % 16 == 0
    for dtype in DTYPES:
        want = expected(want_u8, dtype)
        assert torch.equal(gather(a, b, index, 3, dtype, (F,)), want), (dtype, "shifted")
        assert torch.equal(gather(aligned_a, aligned_b, index, 3, dtype, (F,)), want), (dtype, "aligned")
        one = expected(torch.where(inside, a[safe], torch.zeros((), dtype=torch.uint8, device=DEV)), dtype)
        assert torch.equal(gather(a, None, index, 1, dtype, (F,)), one), (dtype, "one source")


# ------------------------------------------------------------------ packed frames
def test_packed_frames_unpack_through_the_slot_table():
    case = cc.Case(401, 70, 2560, (12, 5, 1), 400, "ring", 1, True)
    shape = (5, 64, 8)
    buf = make_buffer(case, obs_shape=shape, packed=True)
    for c in range(len(case.Ks)):
        buf.collect(to_dev(case.calls[c], shape))
        assert_equals_reference(buf, hc.reference(case, c + 1), ("packed", "call", c))
    st = hc.reference(case)
    n = hc.categories(case, st, 4)
    assert n["full"] > 0 and n["start"] > 0 and n["lost"] > 0 and n["crossing"] > 0, n
    index = hc.sample_index(st)
    # (the shared reference state keeps flat frames: history_reference's frames are reshaped before they are unpacked)
    assert_samples_equal_reference(buf, st, index, case.overflow, case.seed, Ts=(1, 4), what="packed", unpack_w=64)
    s = buf.sample(torch.from_numpy(index).to(DEV), torch.float32, history=4)
    assert tuple(s["obs"].shape) == (len(index), 4, 5, 64, 64) and tuple(s["next_obs"].shape) == (len(index), 4, 5, 64, 64)
    missing = (s["slots"] < 0)
    assert missing.any() and not s["obs"][missing].any()  # missing entries are zero frames


# ------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("overflow", cc.MODES)
def test_captured_collect_with_links_replayed_twice(overflow):
    case = cc.Case(403, 70, 2560, (12, 5, 1), cc.SMALL, overflow, 1, True)
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
    st = hc.new_state(case)
    assert_equals_reference(buf, st, "capture alone changes nothing")
    for r in range(2):
        g.replay()
        col.collect_reference(st, case.calls[0], case.stride, case.overflow, case.seed)
        assert_equals_reference(buf, st, ("replay", r))
    assert st["next_ordinal"] > case.capacity and (st["prev"] >= 0).any()
    assert_samples_equal_reference(buf, st, hc.sample_index(st), case.overflow, case.seed, Ts=(4,), dtypes=(torch.float16,), what="replayed")


# ------------------------------------------------------------------ checkpoints
def test_state_dict_round_trip_with_history():
    case = cc.Case(404, 70, 20, (12, 5, 1), cc.SMALL, "random", 1, True)
    a, b = make_buffer(case), make_buffer(case)
    calls = [to_dev(r) for r in case.calls]
    a.collect(calls[0])
    sd = a.state_dict()
    assert {"prev", "chain"} <= set(sd) and sd["config"]["history"] == 4
    b.load_state_dict(sd)
    for r in calls[1:]:
        a.collect(r)
        b.collect(r)
    st = hc.reference(case)
    assert_equals_reference(a, st, "a")
    assert_equals_reference(b, st, "restored")
    idx = torch.from_numpy(hc.sample_index(st)).to(DEV)
    for pad in hc.PADS:
        sa, sb = a.sample(idx, torch.float16, pad=pad), b.sample(idx, torch.float16, pad=pad)
        assert sa.keys() == sb.keys() and tuple(sa["obs"].shape) == (len(idx), 4, case.F)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (pad, k)
    assert_samples_equal_reference(b, st, hc.sample_index(st), case.overflow, case.seed, Ts=(4,), dtypes=(torch.float16,), what="restored")


# ------------------------------------------------------------------ end to end on simple_layout
N_ENVS, LIMIT, CALLS, CAP, T_E2E = 70, 5, (12, 12, 1), 600, 4


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
    vec.reset(seed=3)
    vec.episode_stats["length"].copy_((torch.arange(N_ENVS, device=DEV) * LIMIT // N_ENVS).to(torch.int32))  # staggered
    vec.set_controller(k=4.0, speed=0.4)
    vec.randomize_drive(maneuvers=(0, 1, 3), mode="cycle", ou=dict(theta=0.1, mu=0.0, sigma=0.4, reset=False), seed=9)
    with pytest.raises(ValueError):
        vec.make_sample_buffer(CAP, stride=2, next_obs=True, history=T_E2E)
    buf = vec.make_sample_buffer(CAP, columns=("maneuver", "steer"), stride=1, overflow="ring", next_obs=True, max_rows=12, history=T_E2E)
    assert buf.history == T_E2E and buf.packed == (packing == "bits") and buf.obs_shape == tuple(vec.out["obs"].shape[1:])
    buf.begin(vec.out["obs"])
    st = col.reference_state(CAP, N_ENVS, buf.obs_shape, {"maneuver": np.int32, "steer": np.float64}, next_obs=True, history=True)
    col.reference_begin(st, vec.out["obs"].cpu().numpy())
    keys = ("obs", "reward", "terminated", "truncated", "maneuver", "steer")
    starts = []
    for c, K in enumerate(CALLS):
        roll = vec.alloc_rollout(K, keys=keys)
        vec.drive(None, roll)
        before = {k: v.clone() for k, v in roll.items()}
        buf.collect(roll)
        torch.cuda.synchronize()
        for k in keys:  # the env's rollouts are untouched by a collect
            assert torch.equal(before[k], roll[k]), k
        starts.append(st["next_ordinal"])
        col.collect_reference(st, {k: v.cpu().numpy() for k, v in roll.items()}, 1, "ring", 0)
        assert_equals_reference(buf, st, (packing, "call", c))
    assert st["next_ordinal"] > CAP and st["count"] == CAP  # slots were overwritten
    n = hc.count_kinds(st, T_E2E, "ring", 0, np.array(starts))
    print(packing, n)
    assert n["full"] > 0 and n["start"] > 0 and n["lost"] > 0 and n["crossing"] > 0, n
    assert_samples_equal_reference(buf, st, hc.sample_index(st), "ring", 0, Ts=(1, 2, T_E2E), dtypes=(torch.float32, torch.uint8, torch.float16),
                                   what=packing, unpack_w=64 if packing == "bits" else None)
    s = buf.sample(buf.sample_index(32))
    assert tuple(s["obs"].shape) == (32, T_E2E, vec.n_classes, 64, 64) and s["obs"].dtype == torch.float32
    assert tuple(s["next_obs"].shape) == tuple(s["obs"].shape) and tuple(s["maneuver"].shape) == (32,)
    steer_history = buf.cols["steer"][s["slots"].clamp(min=0)]
    assert tuple(steer_history.shape) == (32, T_E2E) and torch.equal(steer_history[:, 0], s["steer"])
    vec.close()
