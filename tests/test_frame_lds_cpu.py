"""The frame kernels' own LDS plan (plan_frame_lds, tinycarlo_amd/csrc/tc_plan.h) and the one-word list entries of the
register-held camera path (tc_pack.h), on the CPU through a host-compiler shim (tests/frame_lds_shim.py).

The bytes "today's code" gives a frame workgroup -- the plan's upper limit -- are restated in the shim module from
plan_cam_lds and the R_* macros of k_common.h, not taken from the code under test.
"""
import json
import os
import subprocess

import pytest

import big_maps
import frame_lds_shim as fs
from common import CFG, TEST_CFG, load_cfg


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return fs.build_shim(tmp_path_factory.mktemp("tc_frame_lds"))


def bundled_plan(name):
    cfg, path = load_cfg(name)
    with open(os.path.join(os.path.dirname(path), cfg["map"]["json_path"])) as f:
        return cfg, big_maps.expected_plan(json.load(f))


def regions(f, cap_n, total_nodes):
    """byte ranges of the plan, by the stage they are live in"""
    p_bytes = max(3 * max(cap_n, 1) * 8, total_nodes * 8)
    cam = {"nodes": (f["off_p"], f["off_p"] + p_bytes), "flags": (f["off_flg"], f["off_flg"] + max(cap_n, 1)),
           "list": (f["off_list"], f["off_list"] + f["list_bytes"])}
    if f["counters"]:
        cam["counters"] = (f["off_cnt"], f["off_cnt"] + 64)
    ras = {"tables": (f["r_off_tab"], f["r_off_bits"]), "bits": (f["r_off_bits"], f["r_total"])}
    head = (f["head_off"], f["head_off"] + fs.ENTRY * f["head_cap"])
    return cam, ras, head


def assert_disjoint(named):
    items = sorted(named.items(), key=lambda kv: kv[1])
    for (na, a), (nb, b) in zip(items, items[1:]):
        assert a[1] <= b[0], (na, a, nb, b)


def check_plan(f, cap_n, cap_e, total_nodes, limit):
    cam, ras, head = regions(f, cap_n, total_nodes)
    for k in ("off_p", "off_flg", "off_list", "off_cnt", "r_off_tab", "r_off_bits", "head_off"):
        assert f[k] % 16 == 0, (k, f)
    assert_disjoint(cam)
    assert_disjoint(ras)
    assert_disjoint({**cam, "head": head})
    assert_disjoint({**ras, "head": head})
    assert head[1] <= f["total"] and f["head_cap"] >= 8, f
    assert max(r[1] for r in cam.values()) <= f["cam_total"] <= f["head_off"] and f["r_total"] <= f["head_off"], f
    if limit:
        assert f["total"] <= limit, (f, limit)


def test_cfg3_fits_seven_lds_steps(shim):
    """simple_layout at 64x64, thickness 2: 8960 bytes (seven 1280-byte steps, 18 workgroups in a CU's 160 KB) and a head of
    at least 40 entries, where the layout shared with the other kernels takes 10240 bytes (16 per CU)."""
    cfg, plan = bundled_plan("simple_layout")
    assert (plan["total_nodes"], plan["total_edges"], plan["n_layers"], plan["kframe"]) == (282, 264, 5, 5)
    today, head_today, _ = fs.shared_frame_lds(plan, 64, 64)
    assert (today, head_today) == (10240, 44)
    f = fs.handle_frame_lds(shim, plan, 64, 64, 2)
    check_plan(f, plan["cap_n"], plan["cap_e"], plan["total_nodes"], today)
    assert f["total"] <= 8960 and f["head_cap"] >= 40, f
    assert fs.CU_LDS // fs.align_up(f["total"], fs.LDS_STEP) >= 18
    assert not f["counters"] and f["list_bytes"] >= max(4 * plan["cap_e"], 2 * plan["cap_n"]), f
    assert f["list_bytes"] >= shim.pack_list_bytes(plan["cap_n"], plan["cap_e"])
    # the parts: camera stage 8128, raster stage 5248 + 2560, the head behind the larger
    assert (f["cam_total"], f["r_off_bits"], f["r_total"], f["head_off"]) == (8128, 5248, 7808, 8128), f


@pytest.mark.parametrize("thickness", [1, 3, 8])
def test_four_edge_forms_keep_the_full_tables(shim, thickness):
    _, plan = bundled_plan("simple_layout")
    f = fs.handle_frame_lds(shim, plan, 64, 64, thickness)
    assert f["sh"] == 2 and f["r_off_bits"] == fs.align_up(fs.r_tab_bytes(32), 16) == 6784, f
    check_plan(f, plan["cap_n"], plan["cap_e"], plan["total_nodes"], f["limit"])
    g = fs.handle_frame_lds(shim, plan, 64, 64, 2, short_edges_skip=False)  # TC_SHORT_EDGES=1: four edges at thickness 2 as well
    assert g["r_off_bits"] == 6784
    k16 = fs.frame_lds(shim, 300, 300, 900, False, 16, 2, 2560)
    assert k16["r_off_bits"] == fs.align_up(fs.r_tab_bytes(16), 16)


@pytest.mark.parametrize("name", sorted(CFG) + sorted(TEST_CFG))
@pytest.mark.parametrize("res", [(64, 64), (128, 128), (480, 640)])
def test_bundled_maps_never_exceed_the_shared_layout(shim, name, res):
    cfg, plan = bundled_plan(name)
    for thickness in (1, 2, 3):
        for kw in ({}, {"seg_lds": False}, {"seg_lds_limit": 3}, {"seg_lds_limit": 0}):
            f = fs.handle_frame_lds(shim, plan, res[0], res[1], thickness, **kw)
            check_plan(f, plan["cap_n"], plan["cap_e"], plan["total_nodes"], f["limit"])
            if not f["lean"]:  # the shared layout itself, two-int entries and counters: exactly today's bytes and head
                assert f["total"] == f["limit"] and f["counters"] and f["sh"] == 2, f
                break
            # the plan's own need fits below the limit: the clamp never starves the head
            assert f["head_off"] + fs.LIVE_BYTES <= f["limit"], (f, kw)
            if not kw:
                assert f["head_cap"] >= fs.LIVE_BYTES // fs.ENTRY


@pytest.mark.parametrize("name", sorted(big_maps.CASES))
def test_big_map_cases_never_exceed_the_shared_layout(shim, name):
    case = big_maps.CASES[name]
    _, plan = big_maps.case_map(name, 0)
    H, W = case["res"]
    for thickness in (1, 2, 3, 4):
        f = fs.handle_frame_lds(shim, plan, H, W, thickness)
        check_plan(f, plan["cap_n"], plan["cap_e"], plan["total_nodes"], f["limit"])
        assert f["head_off"] + fs.LIVE_BYTES <= f["limit"], f
        if f["windowed"] or not f["lean"]:
            assert f["counters"] and f["list_bytes"] >= max(2 * plan["cap_e"], plan["cap_n"]) * 4 + 16, f


def test_windowed_groups_keep_counters_and_two_int_entries(shim):
    cap_n, cap_e, tn = 700, 900, 700
    old = big_maps.cam_lds(cap_n, cap_e, tn)
    f = fs.frame_lds(shim, cap_n, cap_e, tn, True, 16, 2, 2560)
    assert f["counters"] and f["off_cnt"] == old["off_cnt"] and f["cam_total"] == old["total"], (f, old)
    assert f["list_bytes"] == old["off_cnt"] - old["off_list"]
    check_plan(f, cap_n, cap_e, tn, 0)
    g = fs.frame_lds(shim, cap_n, cap_e, tn, False, 16, 2, 2560)
    assert not g["counters"] and g["cam_total"] < f["cam_total"]


def test_switches_and_reserve(shim):
    base = fs.frame_lds(shim, 282, 264, 282, False, 32, 1, 2560)
    off = fs.frame_lds(shim, 282, 264, 282, False, 32, 1, 2560, seg_lds=False)
    assert off["head_cap"] == 8 and off["total"] == off["head_off"] + fs.LIVE_BYTES
    for n in (0, 3):
        lim = fs.frame_lds(shim, 282, 264, 282, False, 32, 1, 2560, seg_lds_limit=n)
        assert lim["head_cap"] == 8 and lim["total"] == base["total"]
    res = fs.frame_lds(shim, 282, 264, 282, False, 32, 1, 2560, reserve=256)
    assert res["total"] + 256 == base["total"] and res["head_cap"] < base["head_cap"]


def test_packing(shim):
    assert shim.pack_ids() == fs.PACK_IDS and shim.pack_fits(13) and shim.pack_fits(16) and not shim.pack_fits(17)
    assert shim.pack_walk(832) == 0  # exhaustive: edge, target, other < 832
    w = shim.pack(831, 830, 829)
    assert (shim.pack_edge(w), shim.pack_target(w), shim.pack_other(w)) == (831, 830, 829) and 0 <= w < 2 ** 30
    # the comparison the chain replay uses: among entries of one target, the word orders as the edge id
    t = 517
    words = [shim.pack(e, t, (e * 37) % 832) for e in range(832)]
    assert words == sorted(words) and len(set(words)) == 832
    assert shim.pack_list_bytes(282, 264) == 1072 and shim.pack_list_bytes(600, 10) == 1216


def test_sanitized_program(shim, tmp_path):
    """the shim as a stand-alone program (its own main) under -fsanitize=address,undefined: the exhaustive packing walk, lists
    written through buffers of exactly tc_pack_list_bytes, a grid of plans"""
    exe = fs.build_program(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", (r.returncode, r.stdout, r.stderr[-2000:])
