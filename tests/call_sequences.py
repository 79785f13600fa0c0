"""Sequences of call forms on ONE env handle, and their expected run.

The host side of the HIP library carries state from one call to the next (the frame orders and their cost rows, the env
order of single steps, the event and stream of the last K-step call, the scratch rows and their "every pose row empty,
every length 0" invariant, the ring's slot events, the blob stream position, the two device words of a streamed call).
launch() of tinycarlo_hip.hip takes five routes through it.  A *sequence* cuts a timeline of T flat steps with fixed inputs
(feature_ref.case_inputs(5, n, steps=T), from the reset of feature_ref.host_spawns) into ops, each of which must equal the
same steps done one by one -- so the expected run of every sequence is the flat per-step reference:

  S     one step_device (with a controller: drive_step)           fused step kernel (TC_FUSE=0, packed frames: two launches)
  L k   step_multi / drive of k steps, rollout=None               split, not piped: frame kernel on the caller's stream, last
                                                                  frame into the bound obs
  Q k   k steps, a rollout without "obs"                          as L, plus rollout rows
  R k   k steps, alloc_rollout(k, keys="all")                     streamed (chunked under TC_STREAM=0)
  P k   a prepare_step_multi / prepare_drive object made at the   streamed
        START of the sequence, invoked later (one k per sequence)
  X k   an R op under torch.cuda.stream(side), no host            the `have_call && last_stream != main` wait
        synchronisation around it; the next op is on the default
        stream again
  G k   replay of a torch.cuda.graph captured from an R op that   capture of a call whose cost_row[0] is set
        is not the handle's first K-step call (one k per sequence)
  N k   k steps with env.no_observation = True for that op only   tc_env_kernel<K, false> alone
  M     env.reset(seed, mask) of a third of the envs              MODE_RESET with a mask (a host reset between two ops)

k is one of 2, 3, 5, 9 and not monotone over a sequence, so that the scratch grows mid-sequence (inside step_multi) unless
the sequence reserves it up front -- which every sequence with a G or a P does, before the capture / the prepare: growing
the scratch after a capture is a known hazard and stays outside these tests.

Who orders what.  The library orders a K-step call behind the handle's previous K-step call on another stream
(include/tinycarlo_hip.h); "for every other combination of streams the caller orders them".  The GPU runner therefore adds a
stream-side wait (never a host synchronisation) only where a single step or a graph replay meets an X op (an M synchronises
anyway), and leaves every K-step neighbour of an X -- L, Q, R, P, N -- to the library.

`expected(sequence, fmt, feat)` is the run of tests/feature_ref.py's FeatureRef over the timeline (controller noise only for
steps inside a K-step op: a single step of the controller takes none).  The one big-N case (BIG, big_inputs) is compared with
the plain batched oracle by its test.  Host only: no GPU code, and no answer comes from the library under test."""
import collections
import functools
import zlib

import numpy as np

import feature_ref as fr
import orc

KCODE = 5                 # the K = 5 generated map of the variant matrix
N = fr.N_ENVS
CODES = "SLQRPXGNM"
KS = (2, 3, 5, 9)
K_STEP = "LQRPXGN"        # ops that are ONE call of k steps
STREAMED = "RPXG"         # ... whose every frame goes to a rollout
ROWS = "QRPXGN"           # ops with rollout rows (Q and N: without "obs")
BOUND = "SLQN"            # ops after which the bound buffers hold the op's last step, frame included (N: no frame)
M_MASK = np.arange(N) % 3 == 1
M_SEED = 9100             # the j-th M of a sequence resets with seed M_SEED + 100 * j
GEN_SEED = zlib.crc32(b"call-sequences")

Op = collections.namedtuple("Op", "code k")
Sequence = collections.namedtuple("Sequence", "name ops")


def steps_of(op):
    return 1 if op.code == "S" else 0 if op.code == "M" else op.k


def parse(name, text):
    """"R3 L9 S M R5" -> Sequence"""
    ops = []
    for w in text.split():
        ops.append(Op(w[0], int(w[1:]) if len(w) > 1 else 0))
    s = Sequence(name, tuple(ops))
    validate(s)
    return s


def text_of(seq):
    return " ".join(o.code + (str(o.k) if o.k else "") for o in seq.ops)


def total_steps(seq):
    return sum(steps_of(o) for o in seq.ops)


def reserves_up_front(seq):
    return any(o.code in "GP" for o in seq.ops)


def max_k(seq):
    return max(o.k for o in seq.ops if o.code in K_STEP)


def fixed_k(seq, code):
    ks = {o.k for o in seq.ops if o.code == code}
    return ks.pop() if ks else None


def validate(seq, generated=False):
    ops = seq.ops
    assert all(o.code in CODES for o in ops), seq
    for o in ops:
        assert (o.k in KS) if o.code in K_STEP else o.k == 0, (seq.name, o)
    for code in "GP":  # one captured graph / one prepared object per sequence
        assert len({o.k for o in ops if o.code == code}) <= 1, (seq.name, code, "takes one k per sequence")
    firstk = next(i for i, o in enumerate(ops) if o.code in K_STEP)
    if any(o.code == "G" for o in ops):  # captured from a call that is not the handle's first K-step call
        assert ops[firstk].code != "G", seq.name
    if any(o.code == "P" for o in ops):  # made at the start, invoked after other ops, twice at least
        assert ops[0].code != "P" and sum(o.code == "P" for o in ops) >= 2, seq.name
    assert ops[0].code != "M" and ops[-1].code != "M", seq.name
    assert not any(a.code == "M" and b.code == "M" for a, b in zip(ops, ops[1:])), seq.name
    ks = [o.k for o in ops if o.code in K_STEP]
    if len(ks) >= 3:  # not monotone: the largest k neither first nor last
        assert ks != sorted(ks) and ks != sorted(ks, reverse=True), (seq.name, ks)
    if generated:
        assert 8 <= len(ops) <= 14 and 30 <= total_steps(seq) <= 45, (seq.name, len(ops), total_steps(seq))


# the hand-written sequences: the cases the record of the library names, each with a k that is not monotone
HAND = tuple(parse(n, t) for n, t in (
    ("R_L_R", "R3 L9 R5"),            # a streamed call behind a call that drew its last frame on the caller's stream
    ("R_Q_R", "R5 Q9 R3"),
    ("L_R_first", "L5 R9 R2"),        # ... as the handle's first two K-step calls
    ("R_S_R", "R3 S R9 S S R2"),
    ("R_N_R", "R2 N9 R3"),
    ("R_X_L", "R3 X9 L5"),
    ("X_R", "X5 R9 X2 R3"),
    ("R_G_L_G", "R3 G5 L9 G5"),
    ("P_L_P", "R2 P5 L9 P5 Q2"),
    ("R_M_R", "R3 M R9 L2"),
    ("X_N_X", "R2 X9 N3 X5 R2"),      # a call without observations on either side of a call on another stream
    ("grow", "R2 L3 Q2 R9 L5 R3"),    # no reserve up front: the scratch grows inside the fourth op
))


# observation noise: the blob stream position must advance the same whatever form consumed it
NOISE = parse("noise_R_L_S_R", "R3 L9 S R5")


def required_pairs():
    """every ordered pair of op codes but M M (an M is exempt as a second M)"""
    return {(a, b) for a in CODES for b in CODES} - {("M", "M")}


def pairs_of(seqs):
    return {(a.code, b.code) for s in seqs for a, b in zip(s.ops, s.ops[1:])}


def _walk(rng, n_ops, todo):
    """op codes of one sequence: a walk over the codes that prefers a pair nobody has covered yet"""
    codes, had_k = [], False
    while len(codes) < n_ops:
        prev, last = (codes[-1] if codes else None), len(codes) == n_ops - 1
        cand = [c for c in CODES if not (c == "M" and (prev in (None, "M") or last)) and not (c == "G" and not had_k) and
                not (c == "P" and prev is None)]
        fresh = [c for c in cand if (prev, c) in todo]
        if fresh:
            c = fresh[int(rng.integers(len(fresh)))]
        else:  # towards the code with most uncovered successors
            score = [sum((c, d) in todo for d in CODES) for c in cand]
            best = [c for c, s in zip(cand, score) if s == max(score)]
            c = best[int(rng.integers(len(best)))]
        todo.discard((prev, c))
        codes.append(c)
        had_k |= c in K_STEP
    return codes


def _with_ks(rng, codes):
    """k per op such that the sequence is valid, or None"""
    for _ in range(400):
        kg, kp = (int(rng.choice(KS)) for _ in range(2))
        ops = tuple(Op(c, kg if c == "G" else kp if c == "P" else int(rng.choice(KS)) if c in K_STEP else 0) for c in codes)
        ks = [o.k for o in ops if o.code in K_STEP]
        if 30 <= sum(steps_of(o) for o in ops) <= 45 and (len(ks) < 3 or (ks != sorted(ks) and ks != sorted(ks, reverse=True))):
            return ops
    return None


@functools.lru_cache(maxsize=None)
def generate(seed=GEN_SEED, at_most=24):
    """the seeded generator: sequences of 8 to 14 ops over 30 to 45 steps, made until every required ordered pair of op codes
    occurs in the hand-written and generated sequences together.  Deterministic: numpy's PCG64 stream of (seed, index)."""
    todo = required_pairs() - pairs_of(HAND)
    out, i = [], 0
    while todo and len(out) < at_most:
        rng = np.random.default_rng([seed, i])
        i += 1
        trial = set(todo)
        codes = _walk(rng, int(rng.integers(8, 15)), trial)
        if sum(c == "P" for c in codes) == 1 or sum(c in K_STEP for c in codes) < 3:
            continue
        ops = _with_ks(rng, codes)
        if ops is None:
            continue
        s = Sequence(f"gen{len(out)}", ops)
        validate(s, generated=True)
        todo -= pairs_of([s])
        out.append(s)
    assert not todo, ("the generator did not reach every pair", sorted(todo))
    return tuple(out)


def all_sequences():
    return HAND + generate()


def pair_table(seqs):
    """the table of ordered pairs (rows: first op, columns: second), for failure messages"""
    have = collections.Counter((a.code, b.code) for s in seqs for a, b in zip(s.ops, s.ops[1:]))
    lines = ["    " + "".join(f"{c:>4}" for c in CODES)]
    for a in CODES:
        lines.append(f"{a:>4}" + "".join(f"{have[(a, b)]:>4}" for b in CODES))
    return "\n".join(lines)


# ------------------------------------------------------------------------------------------------- the expected run
def timeline(seq, n=N):
    """car_control [T, n, 2] f64, maneuver [T, n] i32, controller noise [T, n] f64"""
    return fr.case_inputs(KCODE, n, steps=total_steps(seq))


@functools.lru_cache(maxsize=None)
def masked_reset_spawns(seed):
    """what env.reset(seed, mask=M_MASK) draws on the host, from the env's host logic alone (OracleVecEnv: no GPU): the spawn
    nodes of the masked envs and the refilled spawn queue of every env -- the GPU cases hold their env to the same values"""
    from oracle_backend import OracleVecEnv
    oenv = OracleVecEnv(fr.case_cfg(KCODE, True, "classes"), num_envs=N, autoreset=True, spawn="host", spawn_queue_len=fr.QUEUE_LEN)
    oenv.reset(seed=fr.case_seed(KCODE))
    oenv.reset(seed=seed, mask=M_MASK)
    return oenv._keep[0].numpy().copy(), oenv._aux["spawn_queue"].numpy().copy()


def masked_reset(ref, mask, nodes, queue):
    """env.reset(seed, mask) restated on a FeatureRef: the masked envs get a fresh car row (their next episode's), the spawn
    node drawn for them, a running episode of length 0 and no pending re-spawn; EVERY env gets the refilled queue and cursor 0
    (reset(seed=...) re-seeds and refills for the whole batch).  The outputs of the other envs stay their last step's."""
    last = ref.last
    for i in np.flatnonzero(mask):
        if ref.cars:
            ref._draw(i)
        ref.oracles[i].reset(nodes[i:i + 1])
        ref.oracles[i].needs_reset[0] = 0
    for i, o in enumerate(ref.oracles):
        o.spawn_queue = queue[i:i + 1].copy()
        o.spawn_cursor[:] = 0
    if ref.rules is not None:
        ref.rules.reset(mask)
    new = ref._collect(mask, last["steer"])
    for key in ("state", "info", "obs"):  # (info: the time-limit bits of the episode layer live in the last outputs only)
        merged = last[key].copy()
        merged[mask] = new[key][mask]
        new[key] = merged
    return ref._finish(new)


@functools.lru_cache(maxsize=None)
def expected(seq, fmt="classes", feat=0):
    """the expected run of a sequence, computed once per (sequence, format, feature mask) and shared (read only):
    {"reset": out, "steps": [out] * T, "ops": [{"op", "t0", "t1"} | {"op", "t0", "t1", "reset": out, "pending"}],
    "term_counters", "ref"}; fmt: classes | rgb (packed frames are pack_bits_reference of the classes frames)"""
    orc.set_math_mode(orc.MATH_PORTABLE)
    ref = fr.make_reference(KCODE, True, fmt, feat)
    cc, man, noise = timeline(seq)
    run = {"reset": ref.reset(), "steps": [], "ops": [], "ref": ref}
    t = m = 0
    for op in seq.ops:
        if op.code == "M":
            pending = ref.last["needs_reset"].astype(bool).copy()
            out = masked_reset(ref, M_MASK, *masked_reset_spawns(M_SEED + 100 * m))
            run["ops"].append({"op": op, "t0": t, "t1": t, "reset": out, "pending": pending})
            m += 1
            continue
        t0 = t
        for _ in range(steps_of(op)):
            run["steps"].append(ref.step(cc[t], man[t], noise[t] if (feat & fr.FEAT_CTRL and op.code != "S") else None))
            t += 1
        run["ops"].append({"op": op, "t0": t0, "t1": t})
    run["term_counters"] = np.concatenate([o.term_counters for o in ref.oracles])
    return run


def frames_of(out, fmt, n_classes):
    """a step's expected frames [n, bytes] in the env's format (bits: the packed class masks)"""
    obs = out["obs"]
    if fmt == "bits":
        from tinycarlo_amd.packing import pack_bits_reference
        H, W = fr.RES
        return pack_bits_reference(obs.reshape(len(obs), n_classes, H, W)).reshape(len(obs), -1)
    return obs


# ------------------------------------------------------------------------------------- what makes a sequence a test
def boundary_shares(run):
    """per boundary between two ops (step t0 > 0 of an op): the share of envs whose reference frame before differs from the
    frame after, and the shares of non-empty frames on either side -> [(t0, differ, nonempty_before, nonempty_after)]"""
    steps, out = run["steps"], []
    for t0 in sorted({o["t0"] for o in run["ops"] if 0 < o["t0"] < len(steps)}):
        a, b = steps[t0 - 1]["obs"], steps[t0]["obs"]
        out.append((t0, float((a != b).any(axis=1).mean()), float(a.any(axis=1).mean()), float(b.any(axis=1).mean())))
    return out


def respawn_facts(run, feat):
    """-> (an env re-spawns strictly inside a K-step op, an env re-spawns in the first step of an op because the last step of
    the op before ended its episode, a time-limit truncation falls on the last step of an op)"""
    steps = run["steps"]
    inside = first = limit_last = False
    for o in run["ops"]:
        if o["op"].code == "M":
            continue
        t0, t1 = o["t0"], o["t1"]
        if o["op"].code in K_STEP:
            inside |= any(steps[t]["fresh"].any() for t in range(t0 + 1, t1))
        if t0 > 0:
            ended = (steps[t0 - 1]["info"]["terminated"] != 0) | (steps[t0 - 1]["info"]["truncated"] != 0)
            first |= bool((steps[t0]["fresh"] & ended).any())
        if feat & fr.FEAT_EP:
            limit_last |= bool((steps[t1 - 1]["info"]["status"] & fr.S_TIME_LIMIT).any())
    return inside, first, limit_last


# ------------------------------------------------------------------------------------------------ the big-N case
BIG_N = 4096
BIG = parse("big_n", "R9 L5 R9 S S S S S S S S S L3 R5")


def big_inputs(n=BIG_N):
    """bench-like actions (v in 0.3 .. 1, steering in -1 .. 1, float32 like the benchmark's) -> cc [T, n, 2] f32, man [T, n] i32"""
    T = total_steps(BIG)
    rng = np.random.default_rng([GEN_SEED, n])
    cc = np.stack([rng.uniform(0.3, 1.0, (T, n)), rng.uniform(-1.0, 1.0, (T, n))], axis=2).astype(np.float32)
    return cc, rng.integers(0, 4, (T, n)).astype(np.int32)
