"""CPU companions of tests/test_gpu_call_sequences.py: proofs, on the reference alone, that the GPU cases can fail.

  * the sequence generator is deterministic, and every sequence obeys the rules of tests/call_sequences.py;
  * over the whole set every ordered pair of op codes occurs (M is exempt as a second M);
  * every boundary between two ops separates frames that differ, so that a stale or undrawn frame is a mismatch and not a
    coincidence;
  * in every sequence an env re-spawns inside a K-step op, one re-spawns in the first step of an op because the op before
    ended its episode, with episodes a time-limit truncation falls on an op's last step, and every M resets an env that would
    not have re-spawned there."""
import numpy as np
import pytest

import call_sequences as cs
import feature_ref as fr
import orc


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


CASES = [(s, "classes", 0) for s in cs.all_sequences()] + [(s, "classes", 7) for s in cs.HAND] + [(cs.NOISE, "classes", 0)]
IDS = [f"{s.name}-feat{feat}" for s, _, feat in CASES]


def test_generator_is_deterministic_and_obeys_the_rules():
    a = cs.generate()
    cs.generate.cache_clear()
    b = cs.generate()
    assert a == b and [cs.text_of(s) for s in a] == [cs.text_of(s) for s in b]
    assert cs.generate(seed=cs.GEN_SEED + 1) != a, "the seed does not reach the generator"
    cs.generate.cache_clear()
    assert len(a) >= 1
    for s in a:
        cs.validate(s, generated=True)
    for s in cs.HAND:
        cs.validate(s)
    names = [s.name for s in cs.all_sequences()]
    assert len(set(names)) == len(names)
    # the sequences the record of the library names
    texts = {s.name: "".join(o.code for o in s.ops) for s in cs.HAND}
    for want in ("RLR", "RQR", "LR", "RSR", "RNR", "RXL", "XR", "RGLG", "PLP", "RMR", "XNX"):
        assert any(want in t for t in texts.values()), want
    assert texts["L_R_first"].startswith("LR")
    grow = next(s for s in cs.HAND if s.name == "grow")
    ks = [o.k for o in grow.ops if o.code in cs.K_STEP]
    assert not cs.reserves_up_front(grow) and 0 < ks.index(max(ks)) < len(ks) - 1 and ks[0] < max(ks) > ks[-1]


def test_every_ordered_pair_of_ops_occurs():
    seqs = cs.all_sequences()
    missing = cs.required_pairs() - cs.pairs_of(seqs)
    assert not missing, f"pairs without a sequence: {sorted(missing)}\n{cs.pair_table(seqs)}"
    assert ("M", "M") not in cs.pairs_of(seqs)
    print("\n" + cs.pair_table(seqs))


@pytest.mark.parametrize("seq,fmt,feat", CASES, ids=IDS)
def test_boundaries_separate_frames_that_differ(seq, fmt, feat):
    """at every boundary between two ops at least a quarter of the envs have a reference frame before it that differs from the
    frame after it, and at least a quarter of the frames on each side are non-empty.  Achieved on the K = 5 generated map with
    the inputs of feature_ref.case_inputs (MAX_CTE ends a good part of the envs every few steps, the re-spawned car looks at
    another piece of the map; a car that stays moves too little to change its frame): over all sequences the smallest share of
    differing frames is 0.57 at feature mask 0 and 0.38 at mask 7, and every frame on either side of a boundary is non-empty
    (share 1.00)."""
    run = cs.expected(seq, fmt, feat)
    shares = cs.boundary_shares(run)
    assert len(shares) == len({o["t0"] for o in run["ops"]} - {0, cs.total_steps(seq)}) >= 1
    print(f"\n{seq.name} feat {feat}: min differing {min(s[1] for s in shares):.2f}, min non-empty {min(min(s[2:]) for s in shares):.2f}")
    for t0, differ, before, after in shares:
        assert differ >= 0.25, (seq.name, cs.text_of(seq), "boundary at step", t0, differ)
        assert before >= 0.25 and after >= 0.25, (seq.name, "boundary at step", t0, before, after)


@pytest.mark.parametrize("seq,fmt,feat", CASES, ids=IDS)
def test_respawns_fall_where_the_ops_meet(seq, fmt, feat):
    run = cs.expected(seq, fmt, feat)
    assert len(run["steps"]) == cs.total_steps(seq)
    inside, first, limit_last = cs.respawn_facts(run, feat)
    assert inside, (seq.name, "no env re-spawns strictly inside a K-step op")
    assert first, (seq.name, "no env re-spawns in an op's first step because the op before ended its episode")
    if feat & fr.FEAT_EP:
        assert limit_last, (seq.name, "no time-limit truncation on an op's last step")
    else:
        assert not any((s["info"]["status"] & fr.S_TIME_LIMIT).any() for s in run["steps"])
    for o in run["ops"]:
        if o["op"].code == "M":
            assert (cs.M_MASK & ~o["pending"]).any(), (seq.name, "the M resets only envs that would have re-spawned anyway")
            assert o["reset"]["fresh"][cs.M_MASK].all() and not o["reset"]["needs_reset"][cs.M_MASK].any()
            assert (o["reset"]["spawn_cursor"] == 0).all()


def test_masked_reset_of_the_reference_is_the_batched_oracle_env():
    """the restatement of env.reset(seed, mask) on FeatureRef (feature mask 0) against OracleVecEnv, which runs the env's own
    host logic over the batched oracle: state, outputs, pending re-spawns, queue and cursor after R_M_R's steps and reset"""
    import torch
    from oracle_backend import OracleVecEnv
    from tinycarlo_amd import terms as T
    seq = next(s for s in cs.HAND if s.name == "R_M_R")
    run = cs.expected(seq, "classes", 0)
    cc, man, _ = cs.timeline(seq)
    oenv = OracleVecEnv(fr.case_cfg(cs.KCODE, True, "classes"), num_envs=cs.N, autoreset=True, spawn="host", spawn_queue_len=fr.QUEUE_LEN)
    oenv.set_terms([T.cte_termination(fr.MAX_CTE, 1)])
    oenv.reset(seed=fr.case_seed(cs.KCODE))
    m = next(o for o in run["ops"] if o["op"].code == "M")
    for t in range(m["t0"]):
        oenv.step_device(torch.from_numpy(cc[t]), torch.from_numpy(man[t]))
    oenv.reset(seed=cs.M_SEED, mask=cs.M_MASK)
    exp = m["reset"]
    for k in fr.STATE_F:
        assert np.array_equal(oenv.state[k].numpy().view(np.int64), exp["state"][k].view(np.int64)), k
    for k in ("cte", "heading_error", "reward"):
        assert np.array_equal(oenv.out[k].numpy().view(np.int64), exp["info"][k].view(np.int64)), k
    # a reset env has no re-spawn pending (the reset kernel stores 0; the oracle's reset leaves the byte to its caller)
    assert not exp["needs_reset"][cs.M_MASK].any() and m["pending"][cs.M_MASK].any()
    oenv._aux["needs_reset"][torch.from_numpy(cs.M_MASK)] = 0
    assert np.array_equal(oenv._aux["needs_reset"].numpy() != 0, exp["needs_reset"] != 0)
    assert np.array_equal(oenv._aux["spawn_cursor"].numpy(), exp["spawn_cursor"])
    ref = run["ref"]
    assert np.array_equal(oenv._aux["spawn_queue"].numpy(), np.concatenate([o.spawn_queue for o in ref.oracles]))
    g = oenv.out["obs"].numpy().reshape(cs.N, -1)
    assert np.array_equal(g[cs.M_MASK], exp["obs"][cs.M_MASK])
    # and the steps behind it
    for t in range(m["t1"], m["t1"] + 3):
        oenv.step_device(torch.from_numpy(cc[t]), torch.from_numpy(man[t]))
        assert np.array_equal(oenv.out["obs"].numpy().reshape(cs.N, -1), run["steps"][t]["obs"]), t
        assert np.array_equal(oenv.state["x"].numpy().view(np.int64), run["steps"][t]["state"]["x"].view(np.int64)), t


def test_big_n_sequence():
    cs.validate(cs.BIG)
    assert "".join(o.code for o in cs.BIG.ops) == "RLR" + "S" * 9 + "LR"
    assert [o.k for o in cs.BIG.ops if o.code in cs.K_STEP] == [9, 5, 9, 3, 5]
    cc, man = cs.big_inputs()
    assert cc.shape == (cs.total_steps(cs.BIG), cs.BIG_N, 2) and man.shape == cc.shape[:2]
