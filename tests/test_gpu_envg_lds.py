"""The grouped simulate launch sized for what the call reads (plan_envg_lds, tc_plan.h): the lane-line edge records sit in
LDS only when every step computes the distances; otherwise the launch's last step reads them from global memory, and the
per-env distances / term counters are a block of the launch's dynamic LDS sized for the map's layers.

Every case is compared with the CPU oracle at tolerance 0 (the runs of tests/info_rows_ref.py, shared with
tests/test_gpu_info_rows.py where the cases coincide); the drive kernel with the loop of single steps of
tests/test_gpu_controller.py, its reference there.
"""
import numpy as np
import pytest

import envg_lds_shim as es
import orc
from info_rows_ref import reference
from test_gpu_controller import (K as DRIVE_K, assert_final, assert_rows, drive_env, ref, run_drive,  # noqa: F401 (fixtures)
                                 stanley)
from test_gpu_info_rows import INFO, PLAIN, against_oracle, run_gpu
from test_gpu_parity import make_env

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K = 6
KEYS = {"plain": PLAIN, "info": INFO}  # plain: only the last step reads the edge records, from global memory; info: LDS


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def check(monkeypatch, map_name, n, steps, seed, stack, keys, form="streamed", calls=1):
    want = reference(map_name, n, steps * calls, seed, stack)
    snaps = run_gpu(monkeypatch, "0", map_name, n, steps, seed, stack, keys, calls=calls, form=form)
    for c, snap in enumerate(snaps):
        against_oracle(snap, want, c, steps, keys, (map_name, n, steps, form, "call", c))
    return want


@pytest.mark.parametrize("keys", list(KEYS))
@pytest.mark.parametrize("form", ["streamed", "chunked"])
@pytest.mark.parametrize("map_name,n", [("simple_layout", 64), ("simple_layout", 33), ("knuffingen", 64), ("knuffingen", 33)])
def test_both_lds_forms(monkeypatch, map_name, n, form, keys):
    """64 envs: two whole workgroups; 33: the second holds one env.  knuffingen's launch passes the 48 KB default limit in
    either form (its lanepath table alone is 40 KB)."""
    want = check(monkeypatch, map_name, n, K, 4, "none", KEYS[keys], form=form)
    assert (want["nearest_edge"][K - 1] >= 0).any() and (want["laneline_distances"][K - 1] > 0).any()
    assert want["obs"].max() == 255


@pytest.mark.parametrize("keys", list(KEYS))
def test_second_call_on_the_same_handle(monkeypatch, keys):
    check(monkeypatch, "simple_layout", 33, K, 4, "none", KEYS[keys], calls=2)


@pytest.mark.parametrize("stack,keys", [("laneline", "plain"), ("laneline", "info"), ("cte", "plain")])
@pytest.mark.parametrize("form", ["streamed", "chunked"])
def test_terms_count_in_the_dynamic_block(monkeypatch, form, stack, keys):
    """a lane-line stack (every step reads the distances: the LDS copy stays) and a CTE stack (counters without distances:
    the last step's edge scan goes to global memory)"""
    want = check(monkeypatch, "simple_layout", 64, K, 3, stack, KEYS[keys], form=form)
    assert (want["reward"] != 0).any() and (want["term_counters"] != 0).any()


@pytest.mark.parametrize("keys", list(KEYS))
@pytest.mark.parametrize("n", [64, 33])
def test_two_step_call(monkeypatch, n, keys):
    check(monkeypatch, "simple_layout", n, 2, 4, "none", KEYS[keys])


@pytest.mark.parametrize("keys", list(KEYS))
@pytest.mark.parametrize("map_name", ["simple_layout", "knuffingen"])
def test_map_lds_switched_off(monkeypatch, map_name, keys):
    """TC_ENVG_MAP_LDS=0: neither table in LDS whatever the call reads; the per-env block then starts at offset 0"""
    monkeypatch.setenv("TC_ENVG_MAP_LDS", "0")
    check(monkeypatch, map_name, 33, K, 4, "none", KEYS[keys])


def test_drive_kernel_with_every_row(ref):  # noqa: F811
    """tc_drive_envg_kernel, a rollout with distance rows: the LDS copy of the edge records"""
    vec = drive_env()
    assert vec.envg_lds_info(True)["map_in_lds"] == 1
    run_drive(vec, ref, "streamed, every row", "tc_drive_envg_kernel+tc_frame_kernel")
    vec.close()


def test_drive_kernel_without_distance_rows(ref):  # noqa: F811
    """... and one without: the last step's distances, which the env's buffers keep, come from global memory"""
    vec = drive_env()
    info = vec.envg_lds_info(False)
    assert info["map_in_lds"] == 0 and info["static_bytes"] == es.static_lds(ep=True, ctrl=True), info
    roll = vec.alloc_rollout(DRIVE_K, keys=("obs", "reward", "terminated", "truncated", "cte", "heading_error", "status"))
    vec.drive(torch.from_numpy(ref["man"]).cuda(), rollout=roll, steer_noise=torch.from_numpy(ref["noise"]).cuda())
    assert_rows(roll, ref, "streamed, no distance rows")
    assert_final(vec, ref, "streamed, no distance rows")
    vec.close()


def test_info_call_reports_the_launch(monkeypatch):
    """the figures of tc_env_envg_lds_info against the launch's arithmetic restated in tests/envg_lds_shim.py, and the frame
    workgroups beside a simulate workgroup against the value tests/test_envg_lds_cpu.py derives for cfg3's handle"""
    monkeypatch.delenv("TC_ENVG_MAP_LDS", raising=False)
    monkeypatch.delenv("TC_INFO_EVERY_STEP", raising=False)
    n = 64
    env = make_env("simple_layout", "r64", "classes", n)
    frame = env.frame_lds_info()["lds_bytes"]
    edges, lpN, C_ = 264, 187, 5
    for every in (False, True):
        got = env.envg_lds_info(every)
        dyn, map_lds, _ = es.launch_request(edges, lpN, C_, every)
        assert got["dynamic_bytes"] == dyn and bool(got["map_in_lds"]) == map_lds == every, got
        assert got["static_bytes"] == es.static_lds() and got["workgroups"] == n // es.ENVS_PER_WG, got
        granted = es.align_up(dyn + got["static_bytes"], es.LDS_STEP)
        assert got["frames_beside"] == (es.CU_LDS - granted) // es.align_up(frame, es.LDS_STEP), got
    cpu_value = (es.CU_LDS - es.align_up(es.launch_request(edges, lpN, C_, False)[0] + es.static_lds(), es.LDS_STEP)) // 8960
    assert env.envg_lds_info(False)["frames_beside"] >= cpu_value > 14
    env.close()
