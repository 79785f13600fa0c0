"""Per-episode cameras from a bank (tc_env_set_camera_bank, TinyCarloVecEnv.randomize_cameras) against the composed CPU
reference of tests/camera_bank_ref.py, bit for bit: state, info, every frame, the `camera` index rows and the live index /
episode counters.

The settings are the kernel-variant matrix's (tests/feature_ref.py): 37 envs, 64x64 frames, the generated k5_320_nodes map
(fused step kernel; K-step calls through tc_envg_kernel + tc_frame_kernel) and k13_layer_577 map (camera stage inside the
simulate launch, tc_raster_kernel behind it), cte_termination(0.004, 1), a reset, 4 single steps, one 6-step call; the bank
is pitch {10, 14, 19} x fov {90, 110, 129}.  tests/test_camera_bank_cpu.py proves on the reference alone that the call holds
frames whose env has moved on to another camera by the time the call ends -- frames a frame stage reading the env's latest
intrinsics would draw wrong.

Run on the MI355X box with `pytest -m gpu`."""
import numpy as np
import pytest

import camera_bank_ref as cbr
import feature_ref as fr
import orc
import test_gpu_variant_matrix as vm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, NS, NM = cbr.N, cbr.NS, cbr.NM
bits = vm.bits


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


class BankCell(vm.Cell):
    """the matrix's cell with a camera bank installed and compared (no ledger: these cases add no kernel variant)"""

    def __init__(self, kcode, thick, fmt, feat=0, bank=True, single=False, n=N, env_offset=0):
        from tinycarlo_amd import terms as T
        from tinycarlo_amd.vec_env import TinyCarloVecEnv
        self.kcode, self.thick, self.fmt, self.feat = kcode, thick, fmt, feat
        self.label = f"bank kcode {kcode} thick {thick} {fmt} feat {feat}"
        self.plan = fr.case_plan(kcode)
        ref_fmt = "rgb" if fmt == "rgb" else "classes"
        self.run = cbr.reference_run(kcode, thick, ref_fmt, feat, single) if bank else fr.reference_run(kcode, thick, ref_fmt, feat)
        if bank and not single:
            cbr.assert_not_vacuous(cbr.reference_run(kcode, True, "classes"), self.label)
        self.cfg = fr.case_cfg(kcode, thick, fmt)
        self.env = env = TinyCarloVecEnv(self.cfg, num_envs=n, device="cuda:0", autoreset=True, spawn="host",
                                         spawn_queue_len=fr.QUEUE_LEN, obs_packing="bits" if fmt == "bits" else None)
        env.set_terms([T.cte_termination(fr.MAX_CTE, 1)])
        if feat & fr.FEAT_CAR:
            env.randomize_cars(fr.car_ranges_of(env.car_params), seed=fr.CAR_SEED)
        if feat & fr.FEAT_EP:
            env.set_time_limit(None, per_env=fr.case_limits()[0])
        if feat & fr.FEAT_CTRL:
            env.set_controller(k=fr.GAIN, speed=fr.SPEED)
        if bank:
            self.install(single, env_offset)
        cc, man, noise = fr.case_inputs(kcode)
        self.cc, self.man, self.noise = (torch.from_numpy(a).cuda() for a in (cc, man, noise))

    def install(self, single=False, env_offset=0):
        if single:
            self.env.randomize_cameras(fov=[self.cfg["camera"].get("fov", 90)], seed=cbr.CAM_SEED, env_offset=env_offset)
        else:
            self.env.randomize_cameras(seed=cbr.CAM_SEED, env_offset=env_offset, **cbr.BANK)

    def check(self, exp, label, obs=True):
        super().check(exp, label, obs)
        env = self.env
        if "camera" in exp and env.camera_index is not None:
            assert np.array_equal(env.camera_index.cpu().numpy(), exp["camera"]), (self.label, label, "camera_index")
            assert np.array_equal(env.camera_episode.cpu().numpy(), exp["camera_episode"]), (self.label, label, "camera_episode")

    def check_rows(self, roll, steps, label):
        roll = dict(roll)
        cam = roll.pop("camera", None)
        if cam is not None:
            torch.cuda.synchronize()
            want = np.stack([s["camera"] for s in steps])
            assert np.array_equal(cam.cpu().numpy(), want), (self.label, label, "camera rows")
        super().check_rows(roll, steps, label)

    def note(self, n_steps, mode):  # (the plan and the ledger are the matrix's business)
        return self.env.launch_info(n_steps)

    def whole_run(self):
        self.reset()
        self.single_steps()
        return self.call()


CASE1 = [(kc, t, f) for kc in cbr.KCODES for t in (True, False) for f in ("classes", "rgb", "bits")]


@pytest.mark.parametrize("kcode,thick,fmt", CASE1)
def test_bank_against_the_reference(kcode, thick, fmt):
    """case 1: reset + 4 steps + one 6-step call with rollout obs and camera rows, every row compared"""
    c = BankCell(kcode, thick, fmt)
    try:
        assert c.env.camera_bank_params.shape == (cbr.BANK_COUNT, 7) and c.env.camera_episode.sum().item() == 0
        roll_keys = tuple(c.env.alloc_rollout(1, keys="all"))
        assert "camera" in roll_keys
        c.whole_run()
        assert len(np.unique(c.env.camera_index.cpu().numpy())) >= 3
    finally:
        c.close()


SWITCHES = {"chunked": {"TC_STREAM": "0"}, "recover": {"TC_STREAM_TEST_SKIP": "3"}, "two_launch": {"TC_FUSE": "0"},
            "per_env_wavefront": {"TC_ENV_GROUPED": "0"}, "one_fused_launch": {"TC_MULTI_SPLIT": "0"}, "chunk_2": {"TC_STREAM": "0", "TC_CHUNK": "2"}}
CASE2 = [(5, s) for s in SWITCHES] + [(13, "chunked"), (13, "two_launch")]


@pytest.mark.parametrize("kcode,switch", CASE2)
def test_bank_through_the_library_switches(kcode, switch, monkeypatch):
    """case 2: the same run through every form a K-step call can take.  In the recover form the frames with
    (row + env) % 3 == 0 are drawn after the simulate launch has finished -- when every env's live index is its last one"""
    for k, v in SWITCHES[switch].items():
        monkeypatch.setenv(k, v)
    c = BankCell(kcode, True, "classes")
    try:
        frames = c.whole_run()
        if switch == "recover":
            left = (np.arange(NM)[:, None] + np.arange(N)[None, :]) % 3 == 0
            stale = [(j, i) for j, i, _ in cbr.stale_camera_frames(c.run) if left[j, i]]
            assert stale, "no frame of the recover pass belongs to an env that moved on to another camera"
            want = np.stack([c.frames_of(s) for s in c.run["steps"][NS:]])
            assert np.array_equal(frames.reshape(NM, N, -1)[left], want[left])
    finally:
        c.close()


@pytest.mark.parametrize("kcode", cbr.KCODES)
@pytest.mark.parametrize("stream", ("1", "0"))
def test_bank_call_without_rollout_draws_the_last_frame(kcode, stream, monkeypatch):
    """case 2, rollout=None: only the last step's frame is drawn, into the bound observation"""
    monkeypatch.setenv("TC_STREAM", stream)
    c = BankCell(kcode, True, "classes")
    try:
        c.reset()
        c.single_steps()
        c.env.out["obs"].fill_(0xFF)
        c.env.step_multi(c.cc[NS:].contiguous(), c.man[NS:].contiguous())
        c.check(c.run["steps"][-1], "after the call without a rollout", obs=True)
    finally:
        c.close()


@pytest.mark.parametrize("kcode", cbr.KCODES)
def test_drive_with_every_feature_and_the_bank(kcode):
    """case 3: controller + randomize_cars + time limit + bank (feature mask 7) through drive_step and drive"""
    c = BankCell(kcode, True, "classes", feat=7)
    try:
        c.whole_run()
    finally:
        c.close()


def _same(a, b, label):
    for k in a.state:
        assert torch.equal(a.state[k], b.state[k]), (label, k)
    for k in ("cte", "reward", "terminated", "truncated"):
        assert torch.equal(a.out[k], b.out[k]), (label, k)
    assert torch.equal(a.camera_index, b.camera_index) and torch.equal(a.camera_episode, b.camera_episode), label


def test_captured_call_replays_like_eager_and_draws_new_cameras():
    """case 4: a HIP-graph-captured prepare_step_multi replayed twice equals two eager calls; the second replay's episodes
    draw their own cameras"""
    g, e = BankCell(5, True, "classes"), BankCell(5, True, "classes")
    try:
        for c in (g, e):
            c.reset()
        cc, man = g.cc[NS:].contiguous(), g.man[NS:].contiguous()
        keys = ("obs", "reward", "terminated", "camera")
        rg, re_ = g.env.alloc_rollout(NM, keys=keys), e.env.alloc_rollout(NM, keys=keys)
        call = g.env.prepare_step_multi(cc, man, rg)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        seen = []
        for rep in range(2):
            graph.replay()
            e.env.step_multi(cc, man, rollout=re_)
            torch.cuda.synchronize()
            for k in keys:
                assert torch.equal(rg[k], re_[k]), ("replay", rep, k)
            _same(g.env, e.env, f"replay {rep}")
            seen.append((rg["camera"].cpu().numpy().copy(), g.env.camera_episode.cpu().numpy().copy()))
        from tinycarlo_amd.randomization import draw_camera_index
        (rows0, ep0), (rows1, ep1) = seen
        assert (ep1 > ep0).sum() > N // 4, "the second replay re-spawned too few envs"
        assert not np.array_equal(rows0, rows1)
        assert np.array_equal(rows1[-1], draw_camera_index(cbr.CAM_SEED, np.arange(N), ep1 - 1, cbr.BANK_COUNT))
    finally:
        g.close()
        e.close()


def test_state_dict_mid_run_continues_bit_for_bit():
    """case 5: state_dict after the single steps -> a fresh env -> load_state_dict -> the 6-step call equals the reference"""
    a = BankCell(5, True, "classes")
    b = BankCell(5, True, "classes", bank=False)
    b.run = a.run
    try:
        a.reset()
        a.single_steps()
        sd = a.env.state_dict()
        assert set(sd["camera_bank"]) >= {"E", "K", "params", "seed", "env_offset", "index", "episode"}
        assert "camera_bank" not in b.env.state_dict()
        b.env.load_state_dict(sd)
        b.check(a.run["steps"][NS - 1], "after load_state_dict", obs=False)
        assert torch.equal(b.env.camera_index, a.env.camera_index) and b.env.camera_index.data_ptr() != a.env.camera_index.data_ptr()
        b.call()
        a.call()
    finally:
        a.close()
        b.close()


def test_two_shards_equal_one_batch():
    """case 6: envs 0..18 with env_offset 0 and envs 19..36 with env_offset 19 give the rows of the batch of 37"""
    kcode = 5
    run = cbr.reference_run(kcode, True, "classes")
    nodes, queue = fr.host_spawns(kcode)
    for lo, hi in ((0, 19), (19, N)):
        c = BankCell(kcode, True, "classes", n=hi - lo, env_offset=lo)
        try:
            env = c.env
            env._aux["spawn_queue"].copy_(torch.from_numpy(queue[lo:hi]))
            env.reset_to(nodes[lo:hi])
            for t in range(NS):
                env.step_device(c.cc[t, lo:hi].contiguous(), c.man[t, lo:hi].contiguous())
            roll = env.alloc_rollout(NM, keys=("obs", "cte", "camera"))
            env.step_multi(c.cc[NS:, lo:hi].contiguous(), c.man[NS:, lo:hi].contiguous(), rollout=roll)
            torch.cuda.synchronize()
            for j, s in enumerate(run["steps"][NS:]):
                assert np.array_equal(roll["camera"][j].cpu().numpy(), s["camera"][lo:hi]), (lo, j, "camera")
                assert np.array_equal(bits(roll["cte"][j]), bits(s["info"]["cte"][lo:hi])), (lo, j, "cte")
                assert np.array_equal(roll["obs"][j].cpu().numpy().reshape(hi - lo, -1), s["obs"][lo:hi]), (lo, j, "obs")
            last = run["steps"][-1]
            assert np.array_equal(env.camera_index.cpu().numpy(), last["camera"][lo:hi])
            assert np.array_equal(env.camera_episode.cpu().numpy(), last["camera_episode"][lo:hi])
        finally:
            c.close()


@pytest.mark.parametrize("kcode", cbr.KCODES)
def test_switching_back_to_the_shared_camera_and_to_static_rows(kcode):
    """case 7: randomize_cameras() with no argument gives the frames of a run that never installed a bank; set_env_cameras
    after a bank behaves as before (here: static rows of the config's camera -- the shared-camera frames again -- and the
    bank is gone)"""
    for how in ("clear", "static"):
        c = BankCell(kcode, True, "classes")
        try:
            env = c.env
            env.reset(seed=fr.case_seed(kcode))  # (a reset under the bank: indices drawn, frames of other cameras)
            if how == "clear":
                env.randomize_cameras()
            else:
                cam = env.camera
                env.set_env_cameras(orientation=np.tile(np.asarray(cam.orientation, dtype=np.float64), (N, 1)), fov=np.full(N, float(cam.fov)))
            assert env.camera_index is None and env.camera_episode is None and env.camera_bank_params is None
            with pytest.raises(ValueError):
                env.alloc_rollout(NM, keys=("camera",))
            c.run = fr.reference_run(kcode, True, "classes", 0)
            c.whole_run()
        finally:
            c.close()


@pytest.mark.parametrize("kcode", cbr.KCODES)
def test_bank_of_the_configs_camera_equals_the_shared_camera_run(kcode, monkeypatch):
    """case 8: count == 1 with the config's own camera is the shared-camera run bit for bit -- and the whole-frame cull is
    off under a bank: the run does not change with TC_FRAME_CULL, and the frames equal the reference, which has no cull"""
    plain = fr.reference_run(kcode, True, "classes", 0)
    frames = {}
    for cull in ("1", "0"):
        monkeypatch.setenv("TC_FRAME_CULL", cull)
        c = BankCell(kcode, True, "classes", single=True)
        try:
            assert c.env.camera_bank_params.shape == (1, 7)
            frames[cull] = c.whole_run()
            assert not c.env.camera_index.any().item() and c.env.camera_episode.sum().item() > N
            for x, y in zip(c.run["steps"], plain["steps"]):
                assert np.array_equal(x["obs"], y["obs"]) and x["state"].tobytes() == y["state"].tobytes()
        finally:
            c.close()
    assert np.array_equal(frames["1"], frames["0"])
