"""The LDS of a workgroup of the grouped simulate launch (plan_envg_lds, tinycarlo_amd/csrc/tc_plan.h), on the CPU through a
host-compiler shim (tests/envg_lds_shim.py).

In a streamed call the simulate launch shares its CUs with the frame workgroups for most of the call, so what a simulate
workgroup holds decides how many frame workgroups fit beside it.  The bytes the launch asks for are restated in the shim
module (launch_request, static_lds) from the launch code and the kernel's declarations, not taken from the planner; the frame
workgroup's bytes come from the frame plan (tests/frame_lds_shim.py).
"""
import json
import os
import subprocess

import pytest

import big_maps
import envg_lds_shim as es
import frame_lds_shim as fs
from common import load_cfg

N_BENCH = 4096  # envs of the flagship workload


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return es.build_shim(tmp_path_factory.mktemp("tc_envg_lds"))


@pytest.fixture(scope="module")
def frame_shim(tmp_path_factory):
    return fs.build_shim(tmp_path_factory.mktemp("tc_envg_frame_lds"))


def bundled(name, frame_shim):
    """-> total lane-line edges, lanepath nodes, layers, and the frame workgroup's dynamic LDS at 64x64, thickness 2"""
    cfg, path = load_cfg(name)
    with open(os.path.join(os.path.dirname(path), cfg["map"]["json_path"])) as f:
        m = json.load(f)
    plan = big_maps.expected_plan(m)
    frame = fs.handle_frame_lds(frame_shim, plan, 64, 64, 2)["total"]
    return plan["total_edges"], len(m["lanepath"]["nodes"]), plan["n_layers"], frame


def beside(dynamic, static, frame):
    """frame workgroups on a CU beside one simulate workgroup: both granted in whole 1280-byte steps of the CU's 160 KB"""
    granted = es.align_up(dynamic + static, es.LDS_STEP)
    return (es.CU_LDS - granted) // es.align_up(frame, es.LDS_STEP)


@pytest.mark.parametrize("name", ["simple_layout", "knuffingen"])
@pytest.mark.parametrize("info_every", [False, True])
@pytest.mark.parametrize("feat", [(False, False), (True, False), (True, True)], ids=["plain", "ep", "ep_ctrl"])
def test_plan_is_what_the_launch_requests(shim, frame_shim, name, info_every, feat):
    edges, lpN, C_, frame = bundled(name, frame_shim)
    static = es.static_lds(*feat)
    assert static == shim.envg_static(es.ENVS_PER_WG, *map(int, feat))
    p = es.envg_lds(shim, edges, lpN, C_, N_BENCH, info_every, static_bytes=static, frame_lds=frame)
    want, map_lds, fat_lds = es.launch_request(edges, lpN, C_, info_every)
    assert (p["dynamic"], bool(p["map_lds"]), bool(p["fat_lds"])) == (want, map_lds, fat_lds), p
    assert map_lds == info_every and fat_lds, "both bundled maps fit: edge records below 40 KB, lanepath nodes below 56 KB"
    # the regions the kernel addresses: edge records at 0, fat nodes behind them, the per-env blocks behind both
    assert p["fat_off"] == (es.align_up(edges * es.EDGE_BYTES, 16) if map_lds else 0)
    assert p["grp_off"] % 16 == 0 and p["grp_off"] >= p["fat_off"] + lpN * es.LP_NODE_BYTES
    assert p["cnt_off"] == C_ * 8 and p["grp_stride"] == C_ * 8 + es.MAX_TERMS * 4
    assert p["grp_off"] + es.ENVS_PER_WG * p["grp_stride"] <= p["dynamic"]
    assert p["workgroups"] == N_BENCH // es.ENVS_PER_WG == 128
    assert p["static_bytes"] == static and p["granted"] == es.align_up(want + static, es.LDS_STEP)
    assert p["frames_beside"] == beside(want, static, frame), p


def test_simple_layout_default_call_leaves_room_for_sixteen(shim, frame_shim):
    """cfg3: a frame workgroup takes 8960 bytes, 18 to an empty CU.  With the edge records (12.4 KB) and the full-size static
    per-env blocks (5 KB) a simulate workgroup took 36 KB and left room for 14; a default call (no step but the last reads
    distances) now holds the lanepath table and 72 bytes per env."""
    edges, lpN, C_, frame = bundled("simple_layout", frame_shim)
    assert (edges, lpN, C_, frame) == (264, 187, 5, 8960)
    static = es.static_lds()
    want, map_lds, _ = es.launch_request(edges, lpN, C_, False)
    assert not map_lds
    # what the launch took before: edge records + fat nodes dynamic; static 32 x (16 doubles + 8 ints) and the camera indices
    before = beside(es.align_up(edges * 48, 16) + lpN * 96, es.ENVS_PER_WG * (16 * 8 + 8 * 4) + static, frame)
    assert before == 14
    reach = beside(want, static, frame)
    assert es.align_up(want + static, es.LDS_STEP) <= es.CU_LDS - 16 * es.align_up(frame, es.LDS_STEP) == 20480
    assert reach == 16 > before
    p = es.envg_lds(shim, edges, lpN, C_, N_BENCH, False, static_bytes=static, frame_lds=frame)
    assert p["frames_beside"] == reach and not p["map_lds"], p
    # a call that reads distances in every step keeps the copy, and pays for it
    q = es.envg_lds(shim, edges, lpN, C_, N_BENCH, True, static_bytes=static, frame_lds=frame)
    assert q["map_lds"] and q["dynamic"] == p["dynamic"] + es.align_up(edges * 48, 16) and q["frames_beside"] == 14, q


def test_switch_off_and_tables_too_large(shim):
    off = es.envg_lds(shim, 264, 187, 5, 33, True, map_switch=False, frame_lds=8960)
    assert not off["map_lds"] and not off["fat_lds"] and off["grp_off"] == 0
    assert off["dynamic"] == es.launch_request(264, 187, 5, True, map_switch=False)[0] == 32 * (40 + 32)
    assert off["workgroups"] == 2
    big = es.envg_lds(shim, 900, 600, 16, 64, True)
    assert not big["map_lds"] and not big["fat_lds"] and big["dynamic"] == 32 * (128 + 32) and big["frames_beside"] == 0
    edge = es.envg_lds(shim, 853, 597, 5, 64, True)  # 40 944 and 57 312 bytes: both just fit
    assert edge["map_lds"] and edge["fat_lds"] and edge["fat_off"] == 40944
    over = es.envg_lds(shim, 854, 598, 5, 64, True)
    assert not over["map_lds"] and not over["fat_lds"]


def test_pad_takes_slots(shim):
    """the experiment builds' pad: every 8960 bytes is one frame workgroup fewer beside the simulate workgroup"""
    base = es.envg_lds(shim, 264, 187, 5, N_BENCH, False, static_bytes=128, frame_lds=8960)
    for k in (1, 2):
        p = es.envg_lds(shim, 264, 187, 5, N_BENCH, False, static_bytes=128, frame_lds=8960, pad=k * 8960)
        assert p["dynamic"] == base["dynamic"] + k * 8960 and p["frames_beside"] == base["frames_beside"] - k


def test_sanitized_program(tmp_path):
    """the shim as a stand-alone program (its own main) under -fsanitize=address,undefined: a grid of plans, each written
    region by region into a buffer of exactly the bytes the plan asks for"""
    exe = es.build_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", (r.returncode, r.stdout, r.stderr[-2000:])
