"""The composed CPU reference of per-episode cameras from a bank (tc_env_set_camera_bank, TinyCarloVecEnv.randomize_cameras).

`CameraBankRef` is tests/feature_ref.py's `FeatureRef` with one more layer: every env holds an index into a bank of cameras
and, at each re-spawn (the reset included), draws the index of its next episode with `randomization.draw_camera_index` and
hands its oracle that camera -- `Camera(bank_camera_config(cfg, params[idx]))`, the host code of `Camera.update_params`.
An oracle renders a step's frame when the step is computed, so every frame is drawn with the camera of the episode it
belongs to: what the library has to reproduce however late in a K-step call it draws the frame.

The second half describes the cases of tests/test_gpu_camera_bank.py (the settings of the kernel-variant matrix: 37 envs,
64x64, the generated k5 / k13 maps, MAX_CTE, 4 single steps and one 6-step call) and the conditions under which they test
something, checked on the reference alone by tests/test_camera_bank_cpu.py.
Test infrastructure only: no GPU code, and no answer comes from the library under test."""
import copy
import ctypes as C
import functools

import numpy as np

import feature_ref as fr
import orc

KCODES = (5, 13)  # k5_320_nodes: fused step kernel, streamed calls through the frame kernel; k13_layer_577: the camera stage
                  # inside the simulate launch and a raster launch behind it
BANK = {"orientation": {"pitch": [10, 14, 19]}, "fov": [90, 110, 129]}
BANK_COUNT = 9
CAM_SEED = 4242
N, NS, NM = fr.N_ENVS, fr.N_SINGLE, fr.N_MULTI


class CameraBankRef(fr.FeatureRef):
    """FeatureRef plus the camera bank.  camera_cfg: the config's camera section; bank: the candidate lists of
    randomization.camera_bank; env_offset: index of env 0 in a larger population.  Outputs gain
    camera [N] (the index in force in that step) and camera_episode [N]."""

    def __init__(self, *args, camera_cfg, bank, cam_seed, env_offset=0, **kw):
        from tinycarlo_amd.camera import Camera
        from tinycarlo_amd.randomization import bank_camera_config, camera_bank
        super().__init__(*args, **kw)
        self.cam_seed, self.env_offset = cam_seed, env_offset
        self.bank_E, self.bank_K, self.bank_params = camera_bank(camera_cfg, **bank)
        self.cameras = [Camera(bank_camera_config(camera_cfg, row)) for row in self.bank_params]
        self.cam_index = np.zeros(self.N, np.int32)
        self.cam_episode = np.zeros(self.N, np.int32)

    def _draw_camera(self, i):
        from tinycarlo_amd.randomization import draw_camera_index
        idx = int(draw_camera_index(self.cam_seed, self.env_offset + i, int(self.cam_episode[i]), len(self.cameras)))
        self.cam_index[i] = idx
        self.cam_episode[i] += 1
        self.oracles[i].set_camera(self.cameras[idx])

    def _finish(self, out):
        out["camera"], out["camera_episode"] = self.cam_index.copy(), self.cam_episode.copy()
        return super()._finish(out)

    def reset(self):
        for i in range(self.N):
            self._draw_camera(i)
        return super().reset()

    def step(self, cc, man, noise=None):
        # (the draw depends on nothing else of the step: made before the oracles re-spawn, like the device before d_reset)
        for i in np.flatnonzero(np.concatenate([o.needs_reset for o in self.oracles])):
            self._draw_camera(int(i))
        return super().step(cc, man, noise)


def make_reference(kcode, thick, fmt, feat, bank=None, cam_seed=CAM_SEED, env_offset=0):
    """feature_ref.make_reference with the bank on top (fmt: classes | rgb)"""
    from tinycarlo_amd.camera import Camera
    from tinycarlo_amd.config import CarParams
    from tinycarlo_amd.map import Map
    from tinycarlo_amd.randomization import car_ranges
    cfg = fr.case_cfg(kcode, thick, fmt)
    m = Map(cfg["map"])
    p = CarParams.from_config(1 / cfg["sim"].get("fps", 30), cfg["car"])
    cam = Camera(copy.deepcopy(cfg["camera"]))
    nodes, queue = fr.host_spawns(kcode)
    cars = None
    if feat & fr.FEAT_CAR:
        lo, hi, mask = car_ranges(p, fr.car_ranges_of(p))
        cars = {"seed": fr.CAR_SEED, "lo": lo, "hi": hi, "mask": mask}
    limit, length0 = fr.case_limits() if feat & fr.FEAT_EP else (None, None)
    ctrl = {"k": fr.GAIN, "speed": fr.SPEED} if feat & fr.FEAT_CTRL else None
    return CameraBankRef(m, p, cam, orc.FMT_RGB if fmt == "rgb" else orc.FMT_CLASSES, nodes, queue, fr.MAX_CTE, cars=cars, limit=limit,
                         length0=length0, ctrl=ctrl, camera_cfg=copy.deepcopy(cfg["camera"]), bank=BANK if bank is None else bank,
                         cam_seed=cam_seed, env_offset=env_offset)


@functools.lru_cache(maxsize=None)
def reference_run(kcode, thick, fmt, feat=0, single=False):
    """the whole run of a case, computed once and shared (read only): reset, NS single steps, NM steps of one call ->
    {"reset": out, "steps": [out] * 10, "ref"}.  single: a bank of one camera, the config's own"""
    orc.set_math_mode(orc.MATH_PORTABLE)
    cfg = fr.case_cfg(kcode, thick, fmt)
    ref = make_reference(kcode, thick, fmt, feat, bank={"fov": [cfg["camera"].get("fov", 90)]} if single else None)
    cc, man, noise = fr.case_inputs(kcode)
    run = {"reset": ref.reset(), "steps": [], "ref": ref}
    for t in range(NS + NM):
        run["steps"].append(ref.step(cc[t], man[t], noise[t] if (feat & fr.FEAT_CTRL and t >= NS) else None))
    return run


def render_with(ref, env, state_row, camera):
    """the frame of env `env` in the state `state_row` (one element of an output's "state") seen through `camera`: a scratch
    oracle of the env's own map and format, capture + render"""
    src = ref.oracles[env]
    o = orc.Oracle(src.map, ref.p, camera, src.cam.format, 1)
    o.state[0] = state_row
    seg, _ = o.segments(0)
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    frame = np.zeros(o.obs_bytes, np.uint8)
    orc.lib().orc_render(o.map.h, C.byref(o.cam), seg.ctypes.data_as(C.POINTER(C.c_int32)), len(seg),
                         frame.ctypes.data_as(C.POINTER(C.c_uint8)))
    return frame


def stale_camera_frames(run):
    """the (row, env, final index) of the K-step call whose frame is non-empty and whose env has re-spawned to ANOTHER camera
    by the END of the call (the index in force at the last row differs from the frame's own -- an env that went A -> B -> A
    does not count): a frame stage that read the env's latest camera instead of the one that came with the pose, at any time
    from the end of the simulate launch on (the recover pass), would draw these with `final index`"""
    multi = run["steps"][NS:]
    final = multi[-1]["camera"]
    found = []
    for j, s in enumerate(multi[:-1]):
        for i in range(N):
            if s["obs"][i].any() and final[i] != s["camera"][i]:
                assert any(t["fresh"][i] for t in multi[j + 1:])  # (an index only changes at a re-spawn)
                found.append((j, i, int(final[i])))
    return found


def assert_not_vacuous(run, label=""):
    """conditions (a)-(d) of the bank's GPU case, on the reference alone"""
    ref, multi = run["ref"], run["steps"][NS:]
    respawns = int(sum(s["fresh"].sum() for s in multi))
    assert respawns > N, (label, "(a) no more than N re-spawns inside the K-step call", respawns)
    stale = stale_camera_frames(run)
    assert len(stale) >= 8, (label, "(b) fewer than 8 frames whose env ends the call on another camera", len(stale))
    for j, i, later in stale:
        s = multi[j]
        now = render_with(ref, i, s["state"][i], ref.cameras[int(s["camera"][i])])
        assert np.array_equal(now, s["obs"][i]), (label, "the re-render with the frame's own camera is not the frame", j, i)
        then = render_with(ref, i, s["state"][i], ref.cameras[later])
        assert not np.array_equal(then, s["obs"][i]), (label, "(c) the later camera draws the same frame", j, i, later)
    assert len(np.unique(multi[-1]["camera"])) >= 3, (label, "(d) fewer than 3 distinct cameras in force at the last row")
    return respawns, len(stale)
