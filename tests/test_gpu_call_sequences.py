"""One env handle driven from one call form into another, against the flat per-step reference.

Every other GPU test keeps to one call form per handle (or single steps, then one streamed call).  The host side of the HIP
library carries state across calls -- frame orders and cost rows, the env order of single steps, the event and stream of the
last K-step call, scratch rows that every call must leave empty, ring slot events, the blob stream position -- and launch()
takes five routes through it.  tests/call_sequences.py cuts a timeline of fixed inputs into ops (S L Q R P X G N M: see its
head) and says what each step must give; a case here issues the ops of one sequence on one handle WITHOUT a host
synchronisation between them (a sequence that synchronises between ops cannot see an ordering bug), every op writing into
tensors of its own with every observation buffer filled with 0xFF before, the bound buffers cloned in stream order right
behind each S / L / Q / N op, and compares everything bit for bit after ONE final synchronise, the way
test_gpu_variant_matrix.Cell compares: every rollout row of every Q / R / P / X / G / N op, every clone, and the final state,
outputs, needs_reset, spawn_cursor, term_counters, episode statistics and car rows.

Host synchronisations that remain, by necessity: an M op is a host reset (synchronised on both sides); the capture of a G
op's graph (torch.cuda.graph synchronises when it begins); the growth of the scratch inside a call (the library allocates).
Stream-side waits the runner adds, because the caller owes them (include/tinycarlo_hip.h: the library orders a K-step CALL
behind the handle's previous K-step call on another stream, "for every other combination of streams the caller orders
them"): between an X op and a neighbouring single step or graph replay -- a replay is no call of the library.  The clone
behind an L, Q or N op that an X op follows is skipped instead (it would have to be ordered before the side stream's work,
and that wait would order the calls too); behind an S op it stays, the runner's own wait orders it.

tests/test_call_sequences_cpu.py proves on the reference alone that these cases can fail.
Run on the MI355X box with `pytest -m gpu`."""
import copy
import functools
import os
import types

import numpy as np
import pytest

import call_sequences as cs
import feature_ref as fr
import orc
import test_gpu_variant_matrix as vm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = cs.N


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


@pytest.fixture(autouse=True)
def _own_ledger():
    """Cell.note records launches in the variant matrix's ledger: what these cases launch must not count there"""
    saved = set(vm.LEDGER)
    yield
    vm.LEDGER.clear()
    vm.LEDGER.update(saved)


def snapshot(env):
    """the bound buffers and feature tensors, cloned on the current stream"""
    def cl(d):
        return None if d is None else {k: v.clone() for k, v in d.items()}
    s = types.SimpleNamespace(state=cl(env.state), out=cl(env.out), n_classes=env.n_classes,
                              _aux={k: env._aux[k].clone() for k in ("needs_reset", "spawn_cursor")},
                              episode_stats=cl(env.episode_stats))
    for k in ("env_car_params", "car_episode", "steer_last"):
        v = getattr(env, k)
        setattr(s, k, None if v is None else v.clone())
    return s


class Handle:
    """one env handle (a Cell of the variant matrix on the K = 5 generated map) and the ops of a sequence on it"""

    def __init__(self, seq, fmt, feat, fuse=True):
        self.seq, self.fmt, self.feat, self.fuse = seq, fmt, feat, fuse
        self.cell = vm.Cell(cs.KCODE, True, fmt, feat, fuse=fuse)
        self.env = self.cell.env
        self.cell.label = self.label = f"{seq.name} [{cs.text_of(seq)}] {fmt} feat {feat}"
        self.ctrl = bool(feat & fr.FEAT_CTRL)
        self.exp = cs.expected(seq, "rgb" if fmt == "rgb" else "classes", feat)
        self.cc, self.man, self.nz = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in cs.timeline(seq))
        self.side = torch.cuda.Stream()
        self.done = []      # (op record of the expected run, rollout | None, snapshot | None)
        self.infos = []     # (op record, launch_info right behind the op: its plan, with the scratch as the op found it)

    def close(self):
        self.cell.close()

    # ---- the ops
    def call(self, cc, man, nz, roll):
        if self.ctrl:
            self.env.drive(man, rollout=roll, steer_noise=nz)
        else:
            self.env.step_multi(cc, man, rollout=roll)

    def rollout(self, k, obs):
        env = self.env
        keys = tuple(key for key in env.alloc_rollout(1, keys="all") if obs or key != "obs")
        roll = env.alloc_rollout(k, keys=keys)
        if obs:
            roll["obs"].fill_(0xFF)
        return roll

    def prepare(self):
        """everything an op needs, allocated before the first op: the ops themselves only enqueue"""
        env, seq = self.env, self.seq
        if cs.reserves_up_front(seq):
            env.reserve_steps(cs.max_k(seq))
        self.rolls = [self.rollout(o.k, o.code in cs.STREAMED) if o.code in "QRXN" else None for o in seq.ops]
        self.pbuf = self.gbuf = self.pcall = self.graph = None
        kp, kg = cs.fixed_k(seq, "P"), cs.fixed_k(seq, "G")
        if kp:
            self.pbuf = (torch.zeros_like(self.cc[:kp]), torch.zeros_like(self.man[:kp]), torch.zeros_like(self.nz[:kp]), self.rollout(kp, True))
            cc, man, nz, roll = self.pbuf
            self.pcall = env.prepare_drive(man, roll, nz) if self.ctrl else env.prepare_step_multi(cc, man, roll)
        if kg:
            self.gbuf = (torch.zeros_like(self.cc[:kg]), torch.zeros_like(self.man[:kg]), torch.zeros_like(self.nz[:kg]), self.rollout(kg, True))
        torch.cuda.synchronize()

    def load(self, buf, t0, t1):
        """the op's inputs into the fixed tensors of the prepared call / the graph, in stream order"""
        buf[0].copy_(self.cc[t0:t1])
        buf[1].copy_(self.man[t0:t1])
        buf[2].copy_(self.nz[t0:t1])
        buf[3]["obs"].fill_(0xFF)

    def issue(self):
        env, ops = self.env, self.exp["ops"]
        main = torch.cuda.current_stream()
        n_m = 0
        for i, rec in enumerate(ops):
            op, t0, t1 = rec["op"], rec["t0"], rec["t1"]
            prev = ops[i - 1]["op"].code if i else None
            nxt = ops[i + 1]["op"].code if i + 1 < len(ops) else None
            roll = snap = None
            if op.code in "SG" and prev == "X":  # (the caller's to order: a single step and a replay are no K-step calls)
                main.wait_stream(self.side)
            if op.code in cs.BOUND:
                env.out["obs"].fill_(0xFF)
            if op.code == "S":
                if self.ctrl:
                    env.drive_step(self.man[t0])
                else:
                    env.step_device(self.cc[t0], self.man[t0])
            elif op.code in "LQRN":
                roll = self.rolls[i]
                env.no_observation = op.code == "N"
                self.call(self.cc[t0:t1], self.man[t0:t1], self.nz[t0:t1], roll)
                env.no_observation = False
            elif op.code == "X":
                roll = self.rolls[i]
                if prev in ("S", "G"):
                    self.side.wait_stream(main)
                with torch.cuda.stream(self.side):
                    self.call(self.cc[t0:t1], self.man[t0:t1], self.nz[t0:t1], roll)
            elif op.code == "P":
                self.load(self.pbuf, t0, t1)
                self.pcall()
                roll = {k: v.clone() for k, v in self.pbuf[3].items()}
            elif op.code == "G":
                self.load(self.gbuf, t0, t1)
                if self.graph is None:  # captured here: behind at least one K-step call of the handle
                    self.graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self.graph):
                        self.call(*self.gbuf)
                self.graph.replay()
                roll = {k: v.clone() for k, v in self.gbuf[3].items()}
            else:  # M: a host reset between two ops
                torch.cuda.synchronize()
                seed = cs.M_SEED + 100 * n_m
                n_m += 1
                env.reset(seed=seed, mask=cs.M_MASK)
                torch.cuda.synchronize()
                nodes, queue = cs.masked_reset_spawns(seed)
                assert np.array_equal(env._keep[0].cpu().numpy(), nodes) and np.array_equal(env._aux["spawn_queue"].cpu().numpy(), queue)
                snap = snapshot(env)
            if op.code in cs.BOUND and (nxt != "X" or op.code == "S"):
                snap = snapshot(env)
            if op.code != "M":  # (host only: plan_call on the handle's present state; a call sizes the scratch before it is issued)
                env.no_observation = op.code == "N"
                self.infos.append((rec, env.launch_info(cs.steps_of(op))))
                env.no_observation = False
            self.done.append((rec, roll, snap))
        torch.cuda.synchronize()

    # ---- the comparison, after the final synchronise
    def frames(self, t, frames):
        return frames[t] if frames is not None else self.cell.frames_of(self.exp["steps"][t])

    def compare(self, frames=None):
        """frames: None | [T] expected frames [N, bytes] from elsewhere than the reference (the noise case)"""
        env, steps, cell = self.env, self.exp["steps"], self.cell
        n_rows = n_snaps = 0
        for rec, roll, snap in self.done:
            op, t0, t1 = rec["op"], rec["t0"], rec["t1"]
            label = f"op {op.code}{op.k or ''} steps {t0}..{t1 - 1}"
            if roll is not None:
                assert ("obs" in roll) == (op.code in cs.STREAMED), label
                cell.check_rows({k: v for k, v in roll.items() if k != "obs"}, steps[t0:t1], label)
                if "obs" in roll:
                    got = roll["obs"].cpu().numpy().reshape(t1 - t0, N, -1)
                    for j in range(t1 - t0):
                        want = self.frames(t0 + j, frames)
                        assert np.array_equal(got[j], want), (self.label, label, "frame of row", j, "differs in envs",
                                                              np.flatnonzero((got[j] != want).any(axis=1))[:8])
                n_rows += t1 - t0
            if snap is not None:
                c2 = copy.copy(cell)
                c2.env = snap
                got = snap.out["obs"].cpu().numpy().reshape(N, -1)
                if op.code == "M":
                    c2.check(rec["reset"], label, obs=False)
                    want = cell.frames_of(rec["reset"])
                    assert np.array_equal(got[cs.M_MASK], want[cs.M_MASK]), (self.label, label, "frames of the reset envs")
                else:
                    c2.check(steps[t1 - 1], label, obs=False)
                    if op.code == "N":
                        assert (got == 0xFF).all(), (self.label, label, "a call without observations wrote the bound observation")
                    else:
                        want = self.frames(t1 - 1, frames)
                        assert np.array_equal(got, want), (self.label, label, "bound obs differs in envs", np.flatnonzero((got != want).any(axis=1))[:8])
                n_snaps += 1
        assert n_rows > 0
        cell.check(steps[-1], "the handle after the sequence", obs=False)
        assert np.array_equal(env.term_counters.cpu().numpy(), self.exp["term_counters"]), (self.label, "term_counters")

    def check_launches(self, stream=True, chunk=16, segments=False, split=True):
        """what every op launched, from the launch_info taken right behind it; Cell.note then holds kernel and kvar to the
        map's plan (split False: TC_MULTI_SPLIT=0, K steps of a byte format are one fused launch, which is no plan of the
        matrix)"""
        env, cell = self.env, self.cell
        assert len(self.infos) == sum(o.code != "M" for o in self.seq.ops)
        for rec, info in self.infos:
            op = rec["op"]
            k, label = cs.steps_of(op), (self.label, f"op {op.code}{op.k or ''} at step {rec['t0']}", info)
            if op.code == "N":
                assert info["kernel"].endswith("env_kernel") and not info["fused"], label
            elif k == 1:
                assert info["fused"] == (self.fuse and self.fmt != "bits"), label
            elif not split:
                assert info["fused"] and info["kernel"].endswith("step_kernel"), label
            elif not self.fuse:
                assert info["kernel"].endswith("+tc_raster_kernel"), label
            elif segments:  # the budget is small enough: the 9-step call ran as several segments
                assert 2 <= info["steps_per_dispatch"] <= min(k, 8), label
            elif stream:
                assert info["steps_per_dispatch"] == k, ("not streamed",) + label
            else:  # chunked: TC_CHUNK steps, or a quarter of the call when that is less (two at least)
                assert info["steps_per_dispatch"] == min(chunk, max(2, (k + 3) // 4)), label
        for k in sorted({cs.steps_of(o) for o in self.seq.ops if o.code not in "MN"}):
            if k == 1 or split:
                cell.note(k, "step")
        for k in sorted({o.k for o in self.seq.ops if o.code == "N"}):
            env.no_observation = True
            cell.note(k, "step")
            env.no_observation = False


def run_sequence(seq, fmt, feat, fuse=True, **launches):
    h = Handle(seq, fmt, feat, fuse=fuse)
    try:
        h.cell.reset()
        h.prepare()
        h.issue()
        h.compare()
        h.check_launches(**launches)
    finally:
        h.close()


@pytest.mark.parametrize("seq", cs.all_sequences(), ids=lambda s: s.name)
def test_sequence_classes(seq):
    """every sequence, hand-written and generated, on byte class masks without features"""
    run_sequence(seq, "classes", 0)


@pytest.mark.parametrize("feat", (0, 7))
@pytest.mark.parametrize("fmt", ("rgb", "bits"))
@pytest.mark.parametrize("seq", cs.HAND, ids=lambda s: s.name)
def test_hand_written_formats_and_features(seq, fmt, feat):
    """the hand-written sequences on rgb and packed frames (no fused step there: S is two launches, K steps always split),
    without features and with per-env cars, episodes with staggered limits and the controller (feature mask 7)"""
    run_sequence(seq, fmt, feat)


SWITCHES = [
    ({"TC_STREAM": "0"}, {"stream": False}),                               # chunked: ring slots and slot events carried across ops
    ({"TC_STREAM": "0", "TC_CHUNK": "2"}, {"stream": False, "chunk": 2}),  # k = 9: five chunks wrap the ring of three inside an op
    ({"TC_STREAM_TEST_SKIP": "3"}, {}),                                    # the recover pass must leave the scratch clean for the NEXT op
    # (the hook above leaves the SAME frames to the recover pass in every call; with no patience at all whoever finds its row
    # empty gives up, so the frames the recover pass draws change from call to call: a row it left filled is the next call's
    # stale frame)
    ({"TC_STREAM_WAIT_US": "0"}, {}),
    ({"TC_STREAM_SCRATCH_MB": None}, {"segments": True}),                  # (scratch_mb()) k = 9 runs as segments that reuse the scratch rows
    # K steps as ONE fused launch: with N, the forms that are not split -- they too wait for a K-step call on another stream
    # (X then L / R) and are the call an X behind them waits for
    ({"TC_MULTI_SPLIT": "0"}, {"split": False}),
    ({"TC_FUSE": "0"}, {"fuse": False}),
    ({"TC_FRAME_ORDER": "0"}, {}),
]


@functools.lru_cache(maxsize=None)
def scratch_mb():
    """TC_STREAM_SCRATCH_MB for the cases whose 9-step calls must run as segments: the largest budget of a halving series under
    which launch_info(9) reports fewer than 9 steps per dispatch for this map and batch (found on a handle of its own)"""
    key, old = "TC_STREAM_SCRATCH_MB", os.environ.get("TC_STREAM_SCRATCH_MB")
    try:
        for mb in ("8", "4", "2", "1", "0.5", "0.25", "0.125", "0.0625"):
            os.environ[key] = mb
            c = vm.Cell(cs.KCODE, True, "classes", 0)
            try:
                c.env.reserve_steps(9)
                spd = c.env.launch_info(9)["steps_per_dispatch"]
            finally:
                c.close()
            if spd < 9:
                return mb
    finally:
        if old is None:
            os.environ.pop(key, None)
        else:
            os.environ[key] = old
    raise AssertionError("no budget of the series cuts a 9-step call into segments")


@pytest.mark.parametrize("switch,launches", SWITCHES, ids=[",".join(f"{k}={v}" for k, v in s.items()) for s, _ in SWITCHES])
@pytest.mark.parametrize("seq", cs.HAND, ids=lambda s: s.name)
def test_hand_written_switches(seq, switch, launches, monkeypatch):
    """the hand-written sequences under the switches that change how a K-step call is carried out"""
    for k, v in switch.items():
        monkeypatch.setenv(k, v if v is not None else scratch_mb())
    launches = dict(launches)
    assert cs.max_k(seq) == 9
    run_sequence(seq, "classes", 0, fuse=launches.pop("fuse", True), **launches)


def test_scratch_budget_cuts_a_nine_step_call_into_segments(monkeypatch):
    """the computed value of TC_STREAM_SCRATCH_MB used above, held to its purpose: with it launch_info(9) reports fewer than 9
    steps per dispatch on this map and batch"""
    monkeypatch.setenv("TC_STREAM_SCRATCH_MB", scratch_mb())
    c = vm.Cell(cs.KCODE, True, "classes", 0)
    try:
        c.env.reserve_steps(9)
        info = c.env.launch_info(9)
        assert 2 <= info["steps_per_dispatch"] < 9 and info["kernel"] == "tc_envg_kernel+tc_frame_kernel", info
    finally:
        c.close()


def test_noise_position_advances_the_same_whatever_form_consumed_it():
    """set_noise(10, 100, seed) over R L S R: every rendered step consumes one position of the blob stream, whichever form
    rendered it.  The oracle composition has no noise layer, so the expected FRAMES of this one case come from the library's
    own single-step path -- a twin handle stepped singly through the same timeline (the technique of
    test_multi_with_fused_noise_equals_single_steps); everything but the frames is still held to the reference."""
    seq, noise = cs.NOISE, (10, 100, 123)
    twin = Handle(seq, "classes", 0)
    h = None
    try:
        twin.cell.reset()
        twin.env.set_noise(*noise)
        frames, steps = [], twin.exp["steps"]
        for t in range(cs.total_steps(seq)):
            twin.env.step_device(twin.cc[t], twin.man[t])
            frames.append(twin.env.out["obs"].cpu().numpy().reshape(N, -1))
        assert all((f != s["obs"]).any() for f, s in zip(frames, steps)), "the noise left a step's frames untouched"
        h = Handle(seq, "classes", 0)
        h.cell.reset()
        h.env.set_noise(*noise)
        h.prepare()
        h.issue()
        h.compare(frames=frames)
    finally:
        twin.close()
        if h is not None:
            h.close()


def test_big_batch_where_both_order_kernels_exist():
    """N = 4096 on simple_layout, 64x64 class masks, against the plain batched oracle: the only shape above the matrix's,
    because both order mechanisms exist only there -- the env order of single steps needs N a multiple of 4 x the CU count, and
    the window in which a streamed call's sort can overtake the frame launch of the call before is the lifetime of one
    N-workgroup launch.  R9 L5 R9, nine single steps (the env order's refresh fires behind K-step calls), L3 R5, without a
    synchronisation.  launch_info does not say whether a handle has an env order or when its refresh ran, so the case holds
    the device to the library's own condition instead (tc_env_create: N a multiple of G = 4 x the CU count with 2 to 4
    workgroups per SIMD, TC_STEP_ORDER at its default of 8): with it the order exists, and its refresh runs on the ninth
    tc_step of the handle -- the last of the nine single steps here, behind three K-step ops."""
    from test_gpu_bench_shapes import check_rows_against_oracle
    from test_gpu_parity import assert_same, make_env, make_oracle
    seq, n = cs.BIG, cs.BIG_N
    env = make_env("simple_layout", "r64", "classes", n, autoreset=True, spawn_queue_len=16)
    try:
        g = 4 * torch.cuda.get_device_properties(0).multi_processor_count
        assert n % g == 0 and 2 <= n // g <= 4 and os.environ.get("TC_STEP_ORDER") is None, (n, g, "no env order of single steps at this N")
        env.reset(seed=0)
        o = make_oracle(env, threads=16)
        o.reset(env._keep[0].cpu().numpy())
        o.spawn_queue = env._aux["spawn_queue"].cpu().numpy()
        cc, man = (torch.from_numpy(a).cuda() for a in cs.big_inputs())
        rolls = [env.alloc_rollout(op.k, keys="all") if op.code == "R" else None for op in seq.ops]
        for r in rolls:
            if r is not None:
                r["obs"].fill_(0xFF)
        torch.cuda.synchronize()
        done, t = [], 0
        for op, roll in zip(seq.ops, rolls):
            k = cs.steps_of(op)
            if op.code != "R":
                env.out["obs"].fill_(0xFF)
            if op.code == "S":
                env.step_device(cc[t], man[t])
            else:
                env.step_multi(cc[t:t + k], man[t:t + k], rollout=roll)
            snap = None
            if op.code != "R":
                snap = types.SimpleNamespace(state={key: v.clone() for key, v in env.state.items()}, out={key: v.clone() for key, v in env.out.items()},
                                             num_envs=n, cursor=env._aux["spawn_cursor"].clone(), needs_reset=env._aux["needs_reset"].clone())
            done.append((op, t, roll, snap))
            t += k
        torch.cuda.synchronize()
        for k in (1, 3, 5, 9):
            info = env.launch_info(k)
            assert (info["kernel"], info["steps_per_dispatch"]) == (("tc_step_kernel", 1) if k == 1 else ("tc_envg_kernel+tc_frame_kernel", k)), info
        n_reset = 0
        for op, t, roll, snap in done:
            k, label = cs.steps_of(op), f"big batch op {op.code}{op.k or ''} at step {t}"
            if roll is not None:
                n_reset += check_rows_against_oracle(env, o, cc[t:t + k], man[t:t + k], roll, orc.F_AUTORESET, label)
                continue
            for j in range(k):
                n_reset += int(o.needs_reset.sum())
                o.step(cc[t + j].cpu().numpy().astype(np.float64), man[t + j].cpu().numpy(), flags=orc.F_AUTORESET)
            assert_same(snap, o, env.n_classes, label=label)
            assert np.array_equal(snap.cursor.cpu().numpy(), o.spawn_cursor) and np.array_equal(snap.needs_reset.cpu().numpy() != 0, o.needs_reset != 0), label
        assert_same(env, o, env.n_classes, check_obs=False, label="big batch: the handle after the sequence")
        assert np.array_equal(env._aux["spawn_cursor"].cpu().numpy(), o.spawn_cursor)
        assert n_reset > 0, "no env re-spawned"
    finally:
        env.close()
