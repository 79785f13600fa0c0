"""Every compiled instantiation of the simulate, frame and raster kernels, run against the composed CPU reference.

The shipped library holds 254 separately compiled kernels of five families (tinycarlo_hip.hip: Kcodes, Kvars, Thicks, Fmts,
FrameFmts, Feats, DriveFeats); `expected_instantiations` writes the set out as the same Cartesian products.  A case of the
matrix drives one cell of it -- one generated map per K code (tests/big_maps.py), N = 37 envs, 64x64 frames, a reset, 4
single steps and one 6-step call, every observation buffer filled with 0xFF before each call -- and compares everything
with tests/feature_ref.py bit for bit: every single step, every rollout row, the bound buffers at the end.

  part A  tc_[drive_]step_kernel (reset, single steps) and tc_[drive_]envg_kernel + tc_frame_kernel (the streamed call),
          kcode x THICK x FMT x FEAT 0..7
  part B  tc_[drive_]env_kernel<K, true, FEAT> + raster (single steps under TC_FUSE=0), <K, false, FEAT> (a call without
          observations; for K != 13 also a call with frames under TC_ENV_GROUPED=0), K x FEAT 0..7
  part C  what is left of the frame side at FEAT = 0: tc_frame_recover_kernel (TC_STREAM_TEST_SKIP=3), tc_raster_kernel
          (TC_FUSE=0) and the packed tc_frame_kernel, kcode x THICK x FMT {classes, bits, rgb}

The ledger.  Every launch a case makes is recorded as (family, K or kcode, THICK or CAM, FMT, FEAT): the family from
launch_info(...)["kernel"], K from its kvar and the plan (a case asserts the plan with big_maps.expected_launch first: it
must not silently run another variant), THICK and FMT from the config, FEAT from the rule of launch() in tinycarlo_hip.hip:

    const unsigned feat = (e->cr.rows ? TC_FEAT_CAR : 0u) | (e->ep.length && mode != MODE_RENDER ? TC_FEAT_EP : 0u) |
                          (e->ct.tab && mode == MODE_STEP ? TC_FEAT_CTRL : 0u);

(car rows installed -> CAR; episodes installed and not a render -> EP; controller installed and a step -> CTRL: a reset of an
env with a controller runs the kernel without the bit).  The last test of the module holds the ledger to the expected set
when the whole module ran; tests/test_variant_matrix_cpu.py holds the expected set to the library's symbol table and the
parametrisation to the expected set, and proves on the reference alone that no case is vacuous.  A template value added
to the build needs its value in the lists below and a case that reaches it, or those tests fail.

Run on the MI355X box with `pytest -m gpu`."""
import itertools
import time

import numpy as np
import pytest

import big_maps as bm
import feature_ref as fr
import orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

# the variants compiled, per template parameter (tinycarlo_hip.hip)
Kcodes = (516, 5, 8, 9)          # (K, RB) pairs of tc_step_kernel / tc_frame_kernel: 516 = K 5 with batches of 16
Kvars = (5, 8, 9, 13)            # tc_env_kernel
Thicks = (True, False)
Bools = (True, False)            # CAM of tc_env_kernel
Fmts = ("classes", "rgb")
FrameFmts = ("classes", "bits", "rgb")
Feats = (0, 1, 2, 3)
DriveFeats = (4, 5, 6, 7)        # the tc_drive_* entry points


def expected_instantiations():
    """(family, K or kcode, THICK or CAM, FMT, FEAT) of every kernel of the five families; None where a family lacks the parameter"""
    s = set()
    for kc, t, f in itertools.product(Kcodes, Thicks, Fmts):
        s |= {("step", kc, t, f, ft) for ft in Feats} | {("drive_step", kc, t, f, ft) for ft in DriveFeats}
    for k, cam in itertools.product(Kvars, Bools):
        s |= {("env", k, cam, None, ft) for ft in Feats} | {("drive_env", k, cam, None, ft) for ft in DriveFeats}
    s |= {("envg", None, None, None, ft) for ft in Feats} | {("drive_envg", None, None, None, ft) for ft in DriveFeats}
    for kc, t, f in itertools.product(Kcodes, Thicks, FrameFmts):
        s |= {("frame", kc, t, f, None), ("frame_recover", kc, t, f, None)}
    s |= {("raster", None, t, f, None) for t, f in itertools.product(Thicks, FrameFmts)}
    return s


EXPECTED = expected_instantiations()
PART_A = [(kc, t, f, ft) for kc in (5, 516, 8, 9) for t in Thicks for f in Fmts for ft in Feats + DriveFeats]
PART_B = [(k, ft) for k in Kvars for ft in Feats + DriveFeats]
PART_C = [(kc, t, f) for kc in (5, 516, 8, 9) for t in Thicks for f in FrameFmts]
LEDGER = set()
TIMES = {}

N, NS, NM = fr.N_ENVS, fr.N_SINGLE, fr.N_MULTI
STATUS_MASK = 3 | fr.S_TIME_LIMIT  # the bits the oracle knows (assert_same: & 3) and the time limit of the episode layer


def planned_entries(part, case):
    """the instantiations a case is there to launch (what it records beyond them, the reset's kernels for instance, is
    extra); tests/test_variant_matrix_cpu.py holds the union over the three parts to EXPECTED without a GPU"""
    s = set()
    if part == "A":
        kc, t, f, ft = case
        s |= {("drive_step" if ft & 4 else "step", kc, t, f, ft), ("drive_envg" if ft & 4 else "envg", None, None, None, ft),
              ("frame", kc, t, f, None)}
    elif part == "B":
        k, ft = case
        s |= {("drive_env" if ft & 4 else "env", k, cam, None, ft) for cam in Bools}
    else:
        kc, t, f = case
        s |= {("frame", kc, t, f, None), ("frame_recover", kc, t, f, None), ("raster", None, t, f, None)}
    return s


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


class Cell:
    """one env handle of a matrix cell and what it is compared with"""

    def __init__(self, kcode, thick, fmt, feat, fuse=True, env_grouped=True):
        from tinycarlo_amd import terms as T
        from tinycarlo_amd.vec_env import TinyCarloVecEnv
        self.kcode, self.thick, self.fmt, self.feat = kcode, thick, fmt, feat
        self.fuse, self.env_grouped = fuse, env_grouped
        self.label = f"kcode {kcode} thick {thick} {fmt} feat {feat}"
        self.plan = fr.case_plan(kcode)
        self.run = fr.reference_run(kcode, thick, "rgb" if fmt == "rgb" else "classes", feat)
        fr.assert_not_vacuous(self.run, feat, self.label)
        self.env = env = TinyCarloVecEnv(fr.case_cfg(kcode, thick, fmt), num_envs=N, device="cuda:0", autoreset=True, spawn="host",
                                         spawn_queue_len=fr.QUEUE_LEN, obs_packing="bits" if fmt == "bits" else None)
        env.set_terms([T.cte_termination(fr.MAX_CTE, 1)])
        if feat & fr.FEAT_CAR:
            env.randomize_cars(fr.car_ranges_of(env.car_params), seed=fr.CAR_SEED)
        if feat & fr.FEAT_EP:
            env.set_time_limit(None, per_env=fr.case_limits()[0])
        if feat & fr.FEAT_CTRL:
            env.set_controller(k=fr.GAIN, speed=fr.SPEED)
        assert env.n_classes == self.plan["n_layers"]
        cc, man, noise = fr.case_inputs(kcode)
        self.cc, self.man, self.noise = (torch.from_numpy(a).cuda() for a in (cc, man, noise))

    def close(self):
        self.env.close()

    # ---- the ledger
    def note(self, n_steps, mode):
        """asserts that a call of n_steps steps takes the path the plan names, and records what it launches"""
        env, plan = self.env, self.plan
        info = env.launch_info(n_steps)
        if env.no_observation:
            want = (plan["kvar"], "tc_env_kernel")
        elif self.fmt == "bits" and n_steps == 1:  # packed class masks have no fused kernel: a single step is two launches
            want = (plan["kvar"], "tc_env_kernel+tc_raster_kernel")
        else:
            want = bm.expected_launch(plan, n_steps, fuse=self.fuse, env_grouped=self.env_grouped)
        drive = env._ctrl is not None
        name = want[1].replace("tc_env", "tc_drive_env").replace("tc_step", "tc_drive_step") if drive else want[1]
        assert (info["kvar"], info["kernel"]) == (want[0], name), (self.label, n_steps, info, plan["scheme"], plan["kframe"])
        feat = (fr.FEAT_CAR if env.env_car_params is not None else 0) | (fr.FEAT_EP if env.episode_stats is not None else 0) | \
            (fr.FEAT_CTRL if drive and mode == "step" else 0)
        pre = "drive_" if feat & fr.FEAT_CTRL else ""
        sim, _, draw = want[1].partition("+")
        if sim == "tc_step_kernel":
            entries = [(pre + "step", 516 if plan["kframe"] == 516 else info["kvar"], self.thick, self.fmt, feat)]
        elif sim == "tc_envg_kernel":
            entries = [(pre + "envg", None, None, None, feat)]
        else:  # CAM: the camera stage runs in the simulate launch, a raster launch behind it
            entries = [(pre + "env", info["kvar"], draw == "tc_raster_kernel", None, feat)]
        if draw == "tc_frame_kernel":
            entries.append(("frame", plan["kframe"], self.thick, self.fmt, None))
        elif draw == "tc_raster_kernel":
            entries.append(("raster", None, self.thick, self.fmt, None))
        for e in entries:
            assert e in EXPECTED, (self.label, e)
        LEDGER.update(entries)
        return info

    # ---- comparisons
    def frames_of(self, exp):
        obs = exp["obs"]
        if self.fmt == "bits":
            from tinycarlo_amd.packing import pack_bits_reference
            H, W = fr.RES
            return pack_bits_reference(obs.reshape(N, self.env.n_classes, H, W)).reshape(N, -1)
        return obs

    def check(self, exp, label, obs=True):
        """the bound buffers and every feature tensor of the env against the expected outputs of a reset / step"""
        env, C = self.env, self.env.n_classes
        label = (self.label, label)
        torch.cuda.synchronize()
        st, inf = exp["state"], exp["info"]
        for k in fr.STATE_F:
            assert np.array_equal(bits(env.state[k]), bits(st[k])), (label, k)
        n = st["lp_len"]
        assert np.array_equal(env.state["lp_len"].cpu().numpy(), n), (label, "lp_len")
        valid = np.arange(8)[None, :] < 2 * n[:, None]
        assert np.array_equal(np.where(valid, env.state["local_path"].cpu().numpy(), -1), np.where(valid, st["lp"], -1)), (label, "local_path")
        assert np.array_equal(env.state["last_maneuver"].cpu().numpy(), st["last_maneuver"]), (label, "last_maneuver")
        for k in ("cte", "heading_error", "reward"):
            assert np.array_equal(bits(env.out[k]), bits(inf[k])), (label, k)
        for k in ("terminated", "truncated"):
            assert np.array_equal(env.out[k].cpu().numpy() != 0, inf[k] != 0), (label, k)
        assert np.array_equal(env.out["status"].cpu().numpy() & STATUS_MASK, inf["status"] & STATUS_MASK), (label, "status")
        assert np.array_equal(bits(env.out["laneline_distances"]), bits(inf["dist"][:, :C].copy())), (label, "laneline_distances")
        assert np.array_equal(env.out["nearest_edge"].cpu().numpy(), inf["nearest_edge"][:, :C]), (label, "nearest_edge")
        assert np.array_equal(env._aux["needs_reset"].cpu().numpy() != 0, exp["needs_reset"] != 0), (label, "needs_reset")
        assert np.array_equal(env._aux["spawn_cursor"].cpu().numpy(), exp["spawn_cursor"]), (label, "spawn_cursor")
        if obs:
            g, w = env.out["obs"].cpu().numpy().reshape(N, -1), self.frames_of(exp)
            assert np.array_equal(g, w), (label, "obs differs in envs", np.flatnonzero((g != w).any(axis=1))[:8])
        if exp["ep"] is not None:
            for k in fr.EP_KEYS:
                assert np.array_equal(bits(env.episode_stats[k]), bits(exp["ep"][k])), (label, "episode", k)
        if exp["car"] is not None:
            assert np.array_equal(bits(env.env_car_params), bits(exp["car"])), (label, "car rows")
            assert np.array_equal(env.car_episode.cpu().numpy(), exp["car_episode"]), (label, "car_episode")
        if exp["steer"] is not None:
            assert np.array_equal(bits(env.steer_last), bits(exp["steer"])), (label, "steer_last")

    def check_rows(self, roll, steps, label):
        C = self.env.n_classes
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in roll.items()}
        for j, exp in enumerate(steps):
            st, inf = exp["state"], exp["info"]
            valid = np.arange(8)[None, :] < 2 * st["lp_len"][:, None]
            want = {"reward": inf["reward"], "cte": inf["cte"], "heading_error": inf["heading_error"],
                    "terminated": (inf["terminated"] != 0).astype(np.uint8), "truncated": (inf["truncated"] != 0).astype(np.uint8),
                    "x": st["x"], "y": st["y"], "theta": st["theta"], "velocity": st["velocity"], "lp_len": st["lp_len"],
                    "laneline_distances": inf["dist"][:, :C].copy(), "nearest_edge": inf["nearest_edge"][:, :C]}
            if exp["ep"] is not None:
                want.update(episode_length=exp["ep"]["length"], episode_return=exp["ep"]["ret"])
            if exp["steer"] is not None:
                want["steer"] = exp["steer"]
            rest = set(host) - set(want) - {"obs", "status", "local_path"}
            assert not rest, (self.label, "rollout keys without a reference", rest)
            for k, w in want.items():
                assert np.array_equal(bits(host[k][j]), bits(w)), (self.label, label, "row", j, k)
            assert np.array_equal(host["status"][j] & STATUS_MASK, inf["status"] & STATUS_MASK), (self.label, label, "row", j, "status")
            assert np.array_equal(np.where(valid, host["local_path"][j], -1), np.where(valid, st["lp"], -1)), (self.label, label, "row", j, "local_path")
            if "obs" in host:
                g, w = host["obs"][j].reshape(N, -1), self.frames_of(exp)
                assert np.array_equal(g, w), (self.label, label, "frame of row", j, "differs in envs", np.flatnonzero((g != w).any(axis=1))[:8])

    # ---- the sequence of a case: reset, NS single steps, one NM-step call
    def reset(self):
        env = self.env
        self.note(1, "reset")
        env.out["obs"].fill_(0xFF)
        env.reset(seed=fr.case_seed(self.kcode))
        nodes, queue = fr.host_spawns(self.kcode)
        assert np.array_equal(env._keep[0].cpu().numpy(), nodes) and np.array_equal(env._aux["spawn_queue"].cpu().numpy(), queue)
        if self.feat & fr.FEAT_EP:
            env.episode_stats["length"].copy_(torch.from_numpy(fr.case_limits()[1]))
        self.check(self.run["reset"], "reset")

    def single_steps(self):
        env = self.env
        for t in range(NS):
            self.note(1, "step")
            env.out["obs"].fill_(0xFF)
            if self.feat & fr.FEAT_CTRL:
                env.drive_step(self.man[t])
            else:
                env.step_device(self.cc[t], self.man[t])
            self.check(self.run["steps"][t], f"single step {t}")
        assert int(env.out["obs"].max()) > 0

    def call(self):
        """the NM-step call with a keys="all" rollout (without "obs" when the env draws none); -> the rollout's frames on the host"""
        env = self.env
        self.note(NM, "step")
        keys = tuple(env.alloc_rollout(1, keys="all"))
        roll = env.alloc_rollout(NM, keys=tuple(k for k in keys if k != "obs" or not env.no_observation))
        assert ("steer" in roll) == bool(self.feat & fr.FEAT_CTRL) and ("episode_return" in roll) == bool(self.feat & fr.FEAT_EP)
        env.out["obs"].fill_(0xFF)
        if "obs" in roll:
            roll["obs"].fill_(0xFF)
        if self.feat & fr.FEAT_CTRL:
            env.drive(self.man[NS:], rollout=roll, steer_noise=self.noise[NS:].contiguous())
        else:
            env.step_multi(self.cc[NS:].contiguous(), self.man[NS:].contiguous(), rollout=roll)
        self.check_rows(roll, self.run["steps"][NS:], f"{NM}-step call")
        self.check(self.run["steps"][-1], f"after the {NM}-step call", obs=False)
        if "obs" in roll:  # the frames went to the rollout: the bound observation is untouched
            assert bool((env.out["obs"] == 0xFF).all()), (self.label, "a rollout call wrote the bound observation")
            return roll["obs"].cpu().numpy()
        return None


@pytest.mark.parametrize("kcode,thick,fmt,feat", PART_A)
def test_fused_and_grouped_kernels(kcode, thick, fmt, feat):
    """part A: tc_[drive_]step_kernel<kcode, thick, fmt, feat> on the reset and the single steps, tc_[drive_]envg_kernel<feat> and
    tc_frame_kernel<kcode, thick, fmt> on the streamed call"""
    c = Cell(kcode, thick, fmt, feat)
    try:
        c.reset()
        c.single_steps()
        c.env.reserve_steps(NM)  # (the scratch of the call: what launch_info reports depends on it)
        info = c.env.launch_info(NM)
        assert info["steps_per_dispatch"] == NM, (c.label, "the call is not streamed", info)
        c.call()
    finally:
        c.close()
    assert planned_entries("A", (kcode, thick, fmt, feat)) <= LEDGER


@pytest.mark.parametrize("K,feat", PART_B)
def test_one_wavefront_per_env_kernels(K, feat, monkeypatch):
    """part B: tc_[drive_]env_kernel<K, true, feat> + raster (single steps, TC_FUSE=0), <K, false, feat> (a call without
    observations on the same handle; K != 13: a call with frames beside the frame kernel, TC_ENV_GROUPED=0, on a second)"""
    monkeypatch.setenv("TC_FUSE", "0")
    c = Cell(K, True, "classes", feat, fuse=False)
    try:
        c.reset()
        c.single_steps()
        c.env.no_observation = True
        c.call()
    finally:
        c.close()
    if K != 13:
        monkeypatch.delenv("TC_FUSE")
        monkeypatch.setenv("TC_ENV_GROUPED", "0")
        c = Cell(K, True, "classes", feat, env_grouped=False)
        try:
            c.reset()
            c.single_steps()
            c.call()
        finally:
            c.close()
    assert planned_entries("B", (K, feat)) <= LEDGER


@pytest.mark.parametrize("kcode,thick,fmt", PART_C)
def test_frame_side_families(kcode, thick, fmt, monkeypatch):
    """part C, FEAT = 0: the streamed call under TC_STREAM_TEST_SKIP=3 -- the gated workgroups of the frames with
    (row + env) % 3 == 0 give up at once and tc_frame_recover_kernel draws them -- and the single steps under TC_FUSE=0
    (tc_raster_kernel<thick, fmt>).  The recover pass has an observable: the rollout is filled with 0xFF before the call, so
    a frame that tc_frame_kernel left alone equals the reference only if the recover pass drew it."""
    monkeypatch.setenv("TC_STREAM_TEST_SKIP", "3")
    c = Cell(kcode, thick, fmt, 0)
    try:
        c.reset()
        c.single_steps()
        c.env.reserve_steps(NM)
        info = c.env.launch_info(NM)
        assert info["steps_per_dispatch"] == NM and info["kernel"] == "tc_envg_kernel+tc_frame_kernel", (c.label, info)
        frames = c.call()  # (every frame compared with the reference)
        left = (np.arange(NM)[:, None] + np.arange(N)[None, :]) % 3 == 0
        want = np.stack([c.frames_of(s) for s in c.run["steps"][NS:]])
        assert want[left].any(), (c.label, "the frames left to the recover pass are all empty")
        assert np.array_equal(frames.reshape(NM, N, -1)[left], want[left])
        LEDGER.add(("frame_recover", c.plan["kframe"], thick, fmt, None))
    finally:
        c.close()
    monkeypatch.delenv("TC_STREAM_TEST_SKIP")
    monkeypatch.setenv("TC_FUSE", "0")
    c = Cell(kcode, thick, fmt, 0, fuse=False)
    try:
        c.reset()
        c.single_steps()
    finally:
        c.close()
    assert planned_entries("C", (kcode, thick, fmt)) <= LEDGER


def test_ledger_is_complete(request):
    """every expected instantiation was launched by some case (only when the whole module ran)"""
    mine = [i for i in request.session.items if i.module is request.module]
    if len(mine) != len(PART_A) + len(PART_B) + len(PART_C) + 1:
        pytest.skip(f"only {len(mine) - 1} of the matrix's {len(PART_A) + len(PART_B) + len(PART_C)} cases were selected: the ledger is not checked")
    missing = EXPECTED - LEDGER
    slow = sorted(TIMES.items(), key=lambda kv: -kv[1])[:3]
    print(f"\nvariant matrix: {len(LEDGER)} of {len(EXPECTED)} instantiations launched; {sum(TIMES.values()):.1f} s in {len(TIMES)} cases, "
          f"slowest {[(k, round(v, 2)) for k, v in slow]}")
    assert not missing, sorted(missing, key=str)
    assert LEDGER == EXPECTED
