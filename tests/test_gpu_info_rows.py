"""Lane-line distances on demand: a K-step call computes `laneline_distances` / `nearest_edge` at every step only where
someone reads them (rollout rows, a lane-line term), else at the last step of each launch (tc_plan.h, CallPlan::info_every).

Every case is compared with the CPU oracle at tolerance 0 (as tests/test_gpu_parity.py does), and runs a second time on a
handle created under TC_INFO_EVERY_STEP=1 (every step computes them, as before the change): both handles must agree bit
for bit on everything the case reads.  The oracle's runs come from tests/info_rows_ref.py, once per case.
"""
import numpy as np
import pytest

import orc
from info_rows_ref import QLEN, STATE_F, inputs, reference, stack_of, world
from test_gpu_parity import make_env

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PLAIN = ("reward", "terminated", "truncated", "obs")     # what alloc_rollout gives by default: nobody reads distances
INFO = PLAIN + ("laneline_distances", "nearest_edge")
OUT_F = ("cte", "heading_error", "reward", "laneline_distances")   # float64 buffers of the env after a call
OUT_I = ("terminated", "truncated", "nearest_edge")
# launch forms: the switches a handle is created under
FORMS = {"streamed": {}, "chunked": {"TC_STREAM": "0"}, "one_wavefront": {"TC_ENV_GROUPED": "0"}, "fused": {"TC_MULTI_SPLIT": "0"}}


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def run_gpu(monkeypatch, every, map_name, n, K, seed, stack, keys, calls=1, form="streamed", no_observation=False, prepared=False):
    """`calls` K-step calls on a fresh handle -> per call, everything a case may read: the rollout's rows and the env's
    buffers after the call"""
    for k in ("TC_STREAM", "TC_ENV_GROUPED", "TC_MULTI_SPLIT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("TC_INFO_EVERY_STEP", every)
    cfg = world(map_name)[0]
    env = make_env(cfg, *((None, None) if isinstance(cfg, dict) else ("r64", "classes")), n, autoreset=True, spawn_queue_len=QLEN)
    terms, wrapped = stack_of(stack, env.layer_names)
    env.wrapped = wrapped
    if terms:
        env.set_terms(terms)
    env.no_observation = no_observation
    nodes, queue, cc, man = inputs(map_name, n, K * calls, seed)
    env._aux["spawn_queue"].copy_(torch.from_numpy(queue))
    env._aux["spawn_cursor"].zero_()
    env._aux["needs_reset"].zero_()
    env.reset_to(nodes)
    cc_t, man_t = torch.from_numpy(cc).cuda(), torch.from_numpy(man).cuda()
    roll = env.alloc_rollout(K, keys=keys)
    if prepared:  # one object, its tensors refilled between the calls
        cc_b, man_b = cc_t[:K].clone(), man_t[:K].clone()
        call = env.prepare_step_multi(cc_b, man_b, roll)
    snaps = []
    for c in range(calls):
        if prepared:
            cc_b.copy_(cc_t[c * K:(c + 1) * K])
            man_b.copy_(man_t[c * K:(c + 1) * K])
            call()
        else:
            env.step_multi(cc_t[c * K:(c + 1) * K].contiguous(), man_t[c * K:(c + 1) * K].contiguous(), rollout=roll)
        torch.cuda.synchronize()
        s = {("roll", k): roll[k].cpu().numpy().copy() for k in keys}
        s.update({("out", k): env.out[k].cpu().numpy().copy() for k in OUT_F + OUT_I})
        s.update({("state", k): env.state[k].cpu().numpy().copy() for k in STATE_F + ("lp_len", "last_maneuver")})
        s.update({("aux", k): env._aux[k].cpu().numpy().copy() for k in ("needs_reset", "spawn_cursor")})
        s[("aux", "term_counters")] = env.term_counters.cpu().numpy().copy()
        snaps.append(s)
    env.close()
    return snaps


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(got, want, what):
    got, want = bits(got), bits(np.asarray(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), "first at", bad[0].tolist())


def against_oracle(snap, ref, c, K, keys, label):
    """call c (steps c * K .. c * K + K - 1 of the oracle's run): the rows of every step, the env's buffers of the last"""
    t = c * K + K - 1
    n = snap[("out", "cte")].shape[0]
    for k in keys:
        want = ref[k][c * K:c * K + K]
        same(snap[("roll", k)].reshape(want.shape) if k == "obs" else snap[("roll", k)], want, (label, "rollout", k))
    for k in OUT_F + OUT_I:
        same(snap[("out", k)].reshape(n, -1), ref[k][t].reshape(n, -1), (label, "out", k))
    for k in STATE_F + ("lp_len", "last_maneuver"):
        same(snap[("state", k)], ref["state"][t][k], (label, "state", k))
    for k in ("needs_reset", "spawn_cursor", "term_counters"):
        same(snap[("aux", k)], ref[k][t], (label, k))


def check_case(monkeypatch, map_name, n, K, seed, stack, keys, calls=1, **kw):
    ref = reference(map_name, n, K * calls, seed, stack)
    runs = {every: run_gpu(monkeypatch, every, map_name, n, K, seed, stack, keys, calls=calls, **kw) for every in ("0", "1")}
    for every, snaps in runs.items():
        for c, snap in enumerate(snaps):
            against_oracle(snap, ref, c, K, keys, f"TC_INFO_EVERY_STEP={every}, call {c}")
    for c, (a, b) in enumerate(zip(runs["0"], runs["1"])):
        assert a.keys() == b.keys()
        for k in a:
            same(a[k], b[k], ("on demand against every step", c, k))
    return ref


def test_no_info_rows_two_calls(monkeypatch):
    """the default keys: distances are computed at the call's last step only; the env's buffers and every row equal the
    oracle's, and so does a second call on the same handle (the state carried between calls is intact)"""
    ref = check_case(monkeypatch, "simple_layout", 64, 12, 1, "none", PLAIN, calls=2)
    assert ref["fresh"].any() and (ref["nearest_edge"][11] >= 0).any() and ref["obs"].max() == 255


def test_info_rows_requested(monkeypatch):
    ref = check_case(monkeypatch, "simple_layout", 64, 12, 1, "none", INFO, calls=2)
    assert (ref["laneline_distances"] > 0).any() and (ref["nearest_edge"] == -1).any()


@pytest.mark.parametrize("form", ["streamed", "one_wavefront"])
def test_term_that_reads_distances_without_dist_rows(monkeypatch, form):
    """lane-line rewards and the crossing termination, no distance rows: reward and terminated of EVERY step are the
    oracle's (the plan must see the terms and keep the distances on at every step)"""
    ref = check_case(monkeypatch, "simple_layout", 64, 12, 3, "laneline", PLAIN, form=form)
    d = ref["laneline_distances"]
    assert (ref["reward"][:-1] != 0).any() and ref["terminated"].any() and ref["fresh"].any()
    assert len(np.unique(d[:-1][d[:-1] > 0])) > 64, "the lane-line rewards of the steps before the last saw too few distinct distances"


@pytest.mark.parametrize("form", ["streamed", "one_wavefront"])
def test_cte_only_terms_skip_the_distances(monkeypatch, form):
    """a stack that reads no distance: the steps before the last skip them, and reward / terminated must not notice"""
    ref = check_case(monkeypatch, "simple_layout", 64, 12, 3, "cte", PLAIN, form=form)
    assert (ref["reward"] != 0).any() and ref["terminated"][:-1].any() and ref["fresh"].any()


@pytest.mark.parametrize("keys", [PLAIN, INFO], ids=["plain", "info"])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_launch_form(monkeypatch, form, keys):
    check_case(monkeypatch, "simple_layout", 64, 12, 1, "none", keys, form=form)


@pytest.mark.parametrize("keys", [PLAIN, INFO], ids=["plain", "info"])
def test_no_observation(monkeypatch, keys):
    """no frames: the one-wavefront kernel alone, which then also leaves the map window unloaded on the steps it skips"""
    keys = tuple(k for k in keys if k != "obs")
    check_case(monkeypatch, "simple_layout", 64, 12, 1, "none", keys, calls=2, no_observation=True)


def test_prepared_call_replayed(monkeypatch):
    check_case(monkeypatch, "simple_layout", 64, 12, 1, "none", PLAIN, calls=2, prepared=True)


@pytest.mark.parametrize("keys", [PLAIN, INFO], ids=["plain", "info"])
def test_long_call_crosses_a_segment(monkeypatch, keys):
    """300 steps: three streamed segments (128 + 128 + 44 steps), each a launch whose last step computes the distances"""
    check_case(monkeypatch, "simple_layout", 16, 300, 5, "cte", keys)


@pytest.mark.parametrize("map_name,n,K", [("knuffingen", 16, 8), ("big:components_16_layers", 16, 8)])
@pytest.mark.parametrize("keys", [PLAIN, INFO], ids=["plain", "info"])
def test_other_maps(monkeypatch, map_name, n, K, keys):
    """knuffingen (the big bundled map), and a generated map of 16 lane-line layers: four blocks of TC_AG = 5 layers in the
    grouped kernel's distance phase, where the bundled maps (5 layers) have one"""
    ref = check_case(monkeypatch, map_name, n, K, 2, "none", keys)
    assert ref["nearest_edge"].shape[2] == (16 if map_name.startswith("big:") else 5)
    assert (ref["nearest_edge"][-1] >= 0).all(axis=1).any()


# map, envs, K, seed, stack: found on the CPU among seeds 0 .. 63 and K 4 .. 16 with the short CTE termination of the
# "cte" stack -- 9 envs re-spawned at the last step, one on a short path there (the assertions below hold it to that)
LAST = ("simple_layout", 64, 9, 5, "cte")


def test_last_step_without_info(monkeypatch):
    """the call's last step -- the one step whose distances are always computed -- with envs that have none: re-spawned at
    that very step, or on a path of fewer than two nodes (zeros and -1 expected)"""
    map_name, n, K, seed, stack = LAST
    ref = reference(map_name, n, K, seed, stack)
    fresh = ref["fresh"][K - 1]
    short = (ref["lp_len"][K - 1] < 2) & ~fresh
    assert fresh.any() and short.any(), "the case no longer has a re-spawn and a short path at its last step"
    for i in np.flatnonzero(fresh | short):
        assert (ref["nearest_edge"][K - 1][i] == -1).all() and (ref["laneline_distances"][K - 1][i] == 0).all()
    assert (ref["nearest_edge"][K - 1][~(fresh | short)] >= 0).any()
    check_case(monkeypatch, map_name, n, K, seed, stack, PLAIN)
    check_case(monkeypatch, map_name, n, K, seed, stack, PLAIN, form="one_wavefront")
