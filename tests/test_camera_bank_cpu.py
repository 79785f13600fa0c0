"""CPU side of the per-episode camera bank (tc_env_set_camera_bank, TinyCarloVecEnv.randomize_cameras): the draw rule
against the rule written out with the oracle's SplitMix64 and python ints, the bank against `Camera`, the validation, the
header and the binding -- and, on the reference alone, the conditions under which the cases of
tests/test_gpu_camera_bank.py test something (tests/camera_bank_ref.py: assert_not_vacuous)."""
import copy
import os
import re

import numpy as np
import pytest

import camera_bank_ref as cbr
import feature_ref as fr
import orc
from common import ROOT

M64 = (1 << 64) - 1


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def rule(seed, env, episode, count):
    """the issue's rule, with orc_splitmix64_at and python ints"""
    sm = orc.lib().orc_splitmix64_at
    z = sm(sm(seed & M64, 0x63616D), ((env & 0xFFFFFFFF) << 32 | (episode & 0xFFFFFFFF)) & M64)
    return ((z >> 32) * count) >> 32


SEEDS = (0, 1, 0x63616D, 2 ** 63 + 12345, 2 ** 64 - 1)
EDGES = (0, 1, 2 ** 31 - 1, 2 ** 31 + 1, 2 ** 32 - 1)
COUNTS = (1, 2, 400, 2 ** 31)


def test_draw_rule_equals_the_rule_written_out():
    from tinycarlo_amd.randomization import draw_camera_index
    for seed in SEEDS:
        for count in COUNTS:
            for env in EDGES:
                for ep in EDGES:
                    got = int(draw_camera_index(seed, env, ep, count))
                    assert got == rule(seed, env, ep, count), (seed, env, ep, count)
                    assert 0 <= got < count
    # broadcasting: envs down, episodes across
    env, ep = np.array(EDGES, dtype=np.int64)[:, None], np.array(EDGES, dtype=np.int64)[None, :]
    got = draw_camera_index(SEEDS[3], env, ep, 400)
    assert got.shape == (5, 5) and got.dtype == np.int64
    assert got.tolist() == [[rule(SEEDS[3], e, p, 400) for p in EDGES] for e in EDGES]


def test_wrapped_int32_episodes_give_the_same_draw():
    from tinycarlo_amd.randomization import draw_camera_index
    ep = np.array([2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1], dtype=np.int64)
    wrapped = ep.astype(np.uint32).view(np.int32)  # what an int32 counter holds after it passed 2^31 - 1
    assert (wrapped[1:] < 0).all()
    for seed in SEEDS:
        assert np.array_equal(draw_camera_index(seed, 7, ep, 400), draw_camera_index(seed, 7, wrapped, 400))


def test_count_one_gives_zero_and_every_index_occurs():
    from tinycarlo_amd.randomization import draw_camera_index
    env, ep = np.arange(64)[:, None], np.arange(64)[None, :]
    for seed in SEEDS:
        assert not draw_camera_index(seed, env, ep, 1).any()
    got = draw_camera_index(11, np.arange(400)[:, None], np.arange(4096)[None, :], 400)
    assert got.min() == 0 and got.max() == 399 and len(np.unique(got)) == 400
    with pytest.raises(ValueError):
        draw_camera_index(0, 0, 0, 0)


def test_device_header_states_the_same_rule():
    """tc_camera_index of tc_rng.h, built alone by the host compiler, against the host rule"""
    import ctypes as C
    import subprocess
    import tempfile
    from tinycarlo_amd.randomization import draw_camera_index
    with tempfile.TemporaryDirectory() as d:
        src, lib = os.path.join(d, "shim.cpp"), os.path.join(d, "libcam.so")
        with open(src, "w") as f:
            f.write('#include "tc_rng.h"\nextern "C" uint32_t cam_index(uint64_t s, uint32_t e, uint32_t p, uint32_t c) '
                    "{ return tc_camera_index(s, e, p, c); }\n")
        subprocess.check_call(["c++", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"),
                               "-o", lib, src])
        L = C.CDLL(lib)
        L.cam_index.restype = C.c_uint32
        L.cam_index.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
        for seed in SEEDS:
            for count in COUNTS:
                for env in EDGES:
                    for ep in EDGES:
                        assert L.cam_index(seed, env, ep, count) == int(draw_camera_index(seed, env, ep, count)), (seed, env, ep, count)


def _cfg():
    return copy.deepcopy(fr.case_cfg(5, True, "classes")["camera"])


def test_bank_rows_equal_the_camera_bit_for_bit():
    from tinycarlo_amd.camera import Camera
    from tinycarlo_amd.randomization import bank_camera_config, camera_bank
    cfg = _cfg()
    E, K, params = camera_bank(cfg, orientation={"pitch": range(10, 20)}, fov=range(90, 130))
    assert E.shape == (400, 12) and K.shape == (400, 9) and params.shape == (400, 7)
    base = Camera(cfg)
    m = 0
    for pitch in range(10, 20):
        for fov in range(90, 130):
            c = dict(cfg)
            c.update(orientation=[pitch, base.orientation[1], base.orientation[2]], fov=fov)  # the reference's own assignment: ints
            cam = Camera(c)
            assert E[m].tobytes() == cam.E.tobytes() and K[m].tobytes() == cam.K.tobytes(), (pitch, fov)
            assert params[m].tolist() == [pitch, base.orientation[1], base.orientation[2], fov] + [float(v) for v in base.position]
            again = Camera(bank_camera_config(cfg, params[m]))
            assert E[m].tobytes() == again.E.tobytes() and K[m].tobytes() == again.K.tobytes()
            m += 1
    assert len(np.unique(np.concatenate([E, K], axis=1), axis=0)) == 400
    # triples, positions, and every list absent: the config's own camera
    E, K, params = camera_bank(cfg, orientation=[[10, 0, 0], [15, 1, -2]], position=[[0, 0, 0.05], [0.01, 0, 0.06], [0, 0.02, 0.04]])
    assert E.shape == (6, 12) and params[4].tolist() == [15, 1, -2, float(base.fov), 0.01, 0, 0.06]
    for m in range(6):
        cam = Camera(bank_camera_config(cfg, params[m]))
        assert E[m].tobytes() == cam.E.tobytes() and K[m].tobytes() == cam.K.tobytes()
    E, K, params = camera_bank(cfg)
    assert E.shape == (1, 12) and E[0].tobytes() == base.E.tobytes() and K[0].tobytes() == base.K.tobytes()


def test_bank_validation():
    from tinycarlo_amd.randomization import camera_bank
    cfg = _cfg()
    for kw in ({"fov": []}, {"orientation": []}, {"position": []}, {"orientation": {"pitch": []}},
               {"fov": [90, float("nan")]}, {"fov": [float("inf")]}, {"orientation": {"pitch": [10, float("nan")]}},
               {"position": [[0, 0, float("inf")]]}, {"orientation": {"tilt": [1, 2]}}, {"orientation": [[1, 2]]},
               {"fov": [0]}, {"fov": [180]}):
        with pytest.raises(ValueError):
            camera_bank(cfg, **kw)


def test_header_and_binding():
    from tinycarlo_amd import _native
    hdr = open(os.path.join(ROOT, "include", "tinycarlo_hip.h")).read()
    assert re.search(r"^#define TC_HAS_CAMERA_BANK 1$", hdr, re.M)
    assert re.search(r"^#define TC_ABI_VERSION 7$", hdr, re.M) and _native.ABI_VERSION == 7
    assert re.search(r"^int tc_env_set_camera_bank\(tc_env\* env, const tc_camera_bank\* bank\);", hdr, re.M)
    assert "tc_env_set_camera_bank" in _native.EXPORTS and _native.HAS_CAMERA_BANK == 1
    L = _native.lib()
    assert hasattr(L, "tc_env_set_camera_bank") and L.tc_abi_version() == 7
    import ctypes as C
    # tc_camera_bank: 2 pointers, count + env_offset, seed, 2 pointers (the index rows are the call's: tc_step_rows.camera_out)
    assert C.sizeof(_native.CameraBankC) == 2 * 8 + 8 + 8 + 2 * 8
    assert _native.CameraBankC.seed.offset == 24 and _native.CameraBankC.index.offset == 32
    assert _native.CameraBankC.episode.offset == 40 and [n for n, _ in _native.CameraBankC._fields_][-1] == "episode"
    body = re.search(r"typedef struct \{([^}]*)\} tc_camera_bank;", hdr).group(1)
    assert "rows" not in body and _native.StepRows.camera_out.offset == 7 * 8


@pytest.mark.parametrize("kcode", cbr.KCODES)
def test_gpu_case_is_not_vacuous_on_the_reference(kcode):
    """(a)-(d) of the GPU case: enough re-spawns inside the K-step call, frames whose env moves on to another camera later in
    the same call and that the later camera would draw differently, several cameras in force at the end"""
    run = cbr.reference_run(kcode, True, "classes")
    respawns, stale = cbr.assert_not_vacuous(run, f"kcode {kcode}")
    print(f"\nkcode {kcode}: {respawns} re-spawns inside the call, {stale} frames a later camera of the same call would change")
    # the index rows are what draw_camera_index gives for the episode counters, and the counters count every re-spawn
    ref, last = run["ref"], run["steps"][-1]
    total = cbr.N + sum(int(s["fresh"].sum()) for s in run["steps"])
    assert int(last["camera_episode"].sum()) == total
    from tinycarlo_amd.randomization import draw_camera_index
    assert np.array_equal(last["camera"], draw_camera_index(cbr.CAM_SEED, np.arange(cbr.N), last["camera_episode"] - 1, cbr.BANK_COUNT))
    assert len(ref.cameras) == cbr.BANK_COUNT


@pytest.mark.parametrize("kcode", cbr.KCODES)
def test_one_camera_bank_is_the_plain_reference(kcode):
    """a bank of the config's own camera alone changes nothing: the composed reference equals feature_ref's run"""
    a, b = cbr.reference_run(kcode, True, "classes", single=True), fr.reference_run(kcode, True, "classes", 0)
    for x, y in zip([a["reset"]] + a["steps"], [b["reset"]] + b["steps"]):
        assert np.array_equal(x["obs"], y["obs"]) and x["state"].tobytes() == y["state"].tobytes()
        assert x["info"].tobytes() == y["info"].tobytes() and not x["camera"].any()
