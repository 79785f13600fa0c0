"""The host planners of tc_env_create (tinycarlo_amd/csrc/tc_plan.h) on the CPU: the header is built alone by the host
compiler (the shim of tests/big_maps.py) and the planners run on every bundled map, the stress map and the generated
maps of tests/big_maps.py (CASES: 320 .. 2 970 lane-line nodes, up to 16 layers, rings with gaps, dashes, interleaved and
duplicate edges, self-loops, isolated nodes; "<case>/<k>" below is map k of a case).

A plan that reports success is held to the properties the camera stage relies on ("Host structure"); whether
it must report failure is worked out here, independently, from the component sizes of the map.

plan_call, the planner of a call's route through launch(), runs over the full product of its inputs against a restatement
of CallPlan's field comments, its invariants, and the two restatements other tests already hold (at the end of this file).
"""
import ctypes as C

import numpy as np
import pytest

import big_maps
from common import setup

MAX_GROUPS = 8   # TC_MAX_GROUPS
NT = 64          # TC_NT
MAPS = ["simple_layout", "knuffingen", "formula_student_track", "stress_graph"]
BIG = [f"{name}/{k}" for name in big_maps.CASES for k in range(big_maps.N_SEEDS)]  # generated: "<case>/<map of the case>"

@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    return big_maps.build_plan_shim(tmp_path_factory.mktemp("tc_plan"))


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def component_labels(n_nodes, edges):
    """component label of every node (the smallest node id its component holds), -1 = a node without an edge"""
    label = np.arange(n_nodes)
    while True:  # label propagation: every node takes the smallest id its edges reach
        lo = np.minimum(label[edges[:, 0]], label[edges[:, 1]])
        new = label.copy()
        np.minimum.at(new, edges[:, 0], lo)
        np.minimum.at(new, edges[:, 1], lo)
        if np.array_equal(new, label):
            break
        label = new
    has_edge = np.zeros(n_nodes, dtype=bool)
    has_edge[edges.ravel()] = True
    return np.where(has_edge, label, -1)


@pytest.fixture(scope="module")
def graphs():
    """map name -> (node_off, edge_off, edges with global node ids, component label of every node, -1 = no edge)"""
    out = {}
    for name in MAPS:
        f = setup(name)[1].flat()
        node_off, edge_off, edges = big_maps.graph_arrays(f["node_count"], f["edge_count"], f["edges"])
        out[name] = (node_off, edge_off, edges, component_labels(node_off[-1], edges))
    for name in BIG:
        case, k = name.split("/")
        node_off, edge_off, edges = big_maps.graph_of_json(big_maps.case_map(case, int(k))[0])
        out[name] = (node_off, edge_off, edges, component_labels(node_off[-1], edges))
    return out


def _expect_failure(edges, comp, T):
    """why the planner must refuse, worked out from the component sizes alone, or None: a component larger than T; more
    than MAX_GROUPS groups when the components (in order of their first edge) are packed greedily; or groups that are no
    index ranges of the edge list, which is not reordered -- going along it, the group of an edge must never step back"""
    order = list(dict.fromkeys(comp[edges[:, 0]].tolist()))
    nn = {c: int((comp == c).sum()) for c in order}
    ne = {c: int((comp[edges[:, 0]] == c).sum()) for c in order}
    if max(nn.values()) > T or max(ne.values()) > T:
        return "component larger than T"
    group, g, gn, ge = {}, 0, 0, 0
    for c in order:
        if gn + nn[c] > T or ge + ne[c] > T:
            g, gn, ge = g + 1, 0, 0
        group[c] = g
        gn, ge = gn + nn[c], ge + ne[c]
    if max(group.values()) + 1 > MAX_GROUPS:
        return "too many groups"
    if (np.diff([group[c] for c in comp[edges[:, 0]].tolist()]) < 0).any():
        return "groups are not ranges of the edge list"
    return None


@pytest.mark.parametrize("T", [320, 200, 64, 576])
@pytest.mark.parametrize("name", MAPS + BIG)
def test_component_groups(plan, graphs, name, T):
    node_off, edge_off, edges, comp = graphs[name]
    n, te, nl = int(node_off[-1]), int(edge_off[-1]), len(edge_off) - 1
    new_id = np.full(n, -7, dtype=np.int32)
    n0, e0 = np.zeros(MAX_GROUPS + 1, dtype=np.int32), np.zeros(MAX_GROUPS + 1, dtype=np.int32)
    l0, l1 = np.zeros(MAX_GROUPS, dtype=np.int32), np.zeros(MAX_GROUPS, dtype=np.int32)
    caps = np.zeros(2, dtype=np.int32)
    ng = plan.components(_ptr(edge_off), nl, _ptr(edges), n, T, MAX_GROUPS, _ptr(new_id), _ptr(n0), _ptr(e0), _ptr(l0),
                         _ptr(l1), _ptr(caps))
    why = _expect_failure(edges, comp, T)
    if why:
        assert ng == 0, f"{name}, T = {T}: must be refused ({why})"
        return
    assert 1 <= ng <= MAX_GROUPS, f"{name}, T = {T}: nothing stands against a plan, yet the planner refused"
    n0, e0, l0, l1 = n0[:ng + 1], e0[:ng + 1], l0[:ng], l1[:ng]
    used = comp >= 0
    # new_id: -1 off the edges, a bijection onto [0, nodes with an edge) on them
    assert (new_id[~used] == -1).all()
    assert np.array_equal(np.sort(new_id[used]), np.arange(used.sum()))
    # every component is one contiguous run of new ids, its nodes in their old order
    for c in np.unique(comp[used]):
        ids = new_id[comp == c]
        assert np.array_equal(ids, np.arange(ids[0], ids[0] + len(ids))), (name, T, "component", int(c))
    # the groups tile the nodes and the edges without gap or overlap, none larger than T
    assert n0[0] == 0 and n0[-1] == used.sum() and (np.diff(n0) > 0).all()
    assert e0[0] == 0 and e0[-1] == te and (np.diff(e0) > 0).all()
    assert np.diff(n0).max() <= T and np.diff(e0).max() <= T
    assert caps[0] == np.diff(n0).max() and caps[1] == np.diff(e0).max()
    # an edge keeps its index (the edge list is not reordered), and both its ends lie in its own group's node range
    grp_of_edge = np.searchsorted(e0, np.arange(te), side="right") - 1
    for k in range(2):
        ends = new_id[edges[:, k]]
        assert (ends >= n0[grp_of_edge]).all() and (ends < n0[grp_of_edge + 1]).all()
    # ... and the layers a group names are exactly those of its edges
    layer_of_edge = np.searchsorted(edge_off, np.arange(te), side="right") - 1
    for g in range(ng):
        mine = layer_of_edge[e0[g]:e0[g + 1]]
        assert l0[g] == mine.min() and l1[g] == mine.max() + 1


def test_component_groups_cases_are_what_they_are_meant_to_be(graphs):
    """knuffingen is the map that takes component groups: plannable with the default T = 320; T = 64 is less than its
    largest component (checked without the planner), so there the layer scheme must stay"""
    _, _, edges, comp = graphs["knuffingen"]
    assert _expect_failure(edges, comp, 320) is None
    assert _expect_failure(edges, comp, 64) == "component larger than T"
    assert max(int((comp == c).sum()) for c in np.unique(comp[comp >= 0])) > 64


def test_layer_groups_on_knuffingen(plan, graphs):
    node_off, edge_off, _, _ = graphs["knuffingen"]
    nl = len(node_off) - 1
    layer, caps = np.zeros(MAX_GROUPS + 1, dtype=np.int32), np.zeros(2, dtype=np.int32)
    ng = plan.layers(_ptr(node_off), _ptr(edge_off), nl, 9 * NT, MAX_GROUPS, _ptr(layer), _ptr(caps))
    assert ng >= 2
    layer = layer[:ng + 1]
    assert layer[0] == 0 and layer[-1] == nl and (np.diff(layer) > 0).all(), "whole layers, in order"
    largest = max(np.diff(node_off).max(), np.diff(edge_off).max())
    gn, ge = np.diff(node_off[layer]), np.diff(edge_off[layer])
    assert gn.max() <= largest and ge.max() <= largest
    assert caps[0] == gn.max() and caps[1] == ge.max()


@pytest.mark.parametrize("name", BIG)
def test_layer_groups_on_generated_maps(plan, graphs, name):
    """the same properties on the generated maps; whether the planner must refuse is worked out here from the layer sizes:
    a layer beyond the K = 9 cache, or a greedy packing into groups no larger than the largest layer that needs more than
    MAX_GROUPS groups or fewer than two"""
    node_off, edge_off, _, _ = graphs[name]
    nl = len(node_off) - 1
    layer, caps = np.zeros(MAX_GROUPS + 1, dtype=np.int32), np.zeros(2, dtype=np.int32)
    ng = plan.layers(_ptr(node_off), _ptr(edge_off), nl, 9 * NT, MAX_GROUPS, _ptr(layer), _ptr(caps))
    sizes = list(zip(np.diff(node_off).tolist(), np.diff(edge_off).tolist()))
    largest = max(max(s) for s in sizes)
    count, gn, ge = 1, 0, 0
    for n, e in sizes:
        if gn + n > largest or ge + e > largest:
            count, gn, ge = count + 1, 0, 0
        gn, ge = gn + n, ge + e
    if largest > 9 * NT or count > MAX_GROUPS or count < 2:
        assert ng == 0, (name, "must be refused", largest, count)
        return
    assert ng == count
    layer = layer[:ng + 1]
    assert layer[0] == 0 and layer[-1] == nl and (np.diff(layer) > 0).all(), "whole layers, in order"
    gn, ge = np.diff(node_off[layer]), np.diff(edge_off[layer])
    assert gn.max() <= largest and ge.max() <= largest
    assert caps[0] == gn.max() and caps[1] == ge.max()


# ---------------------------------------------------------------------------------------------- plan_call
NO_OBSERVATION = 1       # TC_F_NO_OBSERVATION
NO_FRAME_FLAGS = 0x401   # ... | DBG_SKIP_CAMERA: what the host side passes as no_frame_flags
CHUNKS = (2, 16)
KVARS = (5, 8, 9, 13)
NSTEPS = (1, 2, 3, 5, 9, 20, 64, 200)
RING_ROWS = (0, 2, 16)
STREAMED_ROWS = (0, 1, 2, 9, 128)


@pytest.fixture(scope="module")
def calls(plan):
    """the full product of plan_call's inputs -> (inputs by name, plan_call's answers by name), one array per field"""
    axes = {"fuse": (0, 1), "multi_split": (0, 1), "env_grouped": (0, 1), "pipe": (0, 1), "stream": (0, 1), "chunk": CHUNKS,
            "kvar": KVARS, "packed": (0, 1), "ring_rows": RING_ROWS, "streamed_rows": STREAMED_ROWS, "st_words": (0, 1),
            "flags": (0, NO_OBSERVATION), "no_frame_flags": (NO_FRAME_FLAGS,), "nsteps": NSTEPS, "obs": (0, 1), "all": (0, 1)}
    assert tuple(axes) == big_maps.CALL_INPUTS
    grid = np.meshgrid(*[np.asarray(v, dtype=np.int32) for v in axes.values()], indexing="ij")
    rows = np.stack([g.ravel() for g in grid], axis=1)
    out = big_maps.plan_calls(plan, rows)
    i = dict(zip(big_maps.CALL_INPUTS, rows.T))
    p = dict(zip(big_maps.CALL_PLAN, out.T))
    for k in big_maps.CALL_PLAN[:-1]:
        assert np.isin(p[k], (0, 1)).all()
        p[k] = p[k].astype(bool)
    return i, p


def restated_plan(i):
    """CallPlan restated from its field comments (tc_plan.h), by the form a call takes rather than bit by bit.

    Frames are drawn when there is a tensor and no flag forbids it.  A handle has the frame kernel unless its simulate
    stage is the K = 13 one or TC_FUSE=0; it has the fused step kernel when it has the frame kernel and the format is not
    the packed one.  A call that draws is then one of:
      fused      a single step with the step kernel; K steps with it under TC_MULTI_SPLIT=0
      split      every other K-step call: with the frame kernel (`frames`) or with camera-in-simulate + raster launches
      two        a single step without the step kernel
    A split call with the frame kernel simulates with the grouped kernel under TC_ENV_GROUPED; such a call is piped when
    TC_CHUNK > 0 and every frame is wanted, and a piped call is streamed under TC_STREAM once the scratch of streamed calls
    (two rows at least) and its two device words exist.
    Steps per dispatch: a streamed call, all of them or as many as its scratch has rows; a fused call, all of them;
    a piped chunked call, TC_CHUNK or a quarter of the call (rounded up, two at least), whichever is less; any other
    call, all of them -- and whatever is neither fused nor streamed never more than a slot of the ring holds, when there
    is a ring (tc_env_launch_info reports the two-launch forms so, too)."""
    b = {k: v.astype(bool) for k, v in i.items() if k not in ("chunk", "kvar", "ring_rows", "streamed_rows", "flags", "no_frame_flags", "nsteps")}
    draws = b["obs"] & ((i["flags"] & i["no_frame_flags"]) == 0)
    has_frame_kernel = b["fuse"] & (i["kvar"] != 13)
    has_step_kernel = has_frame_kernel & ~b["packed"]
    k_steps = i["nsteps"] > 1
    form = np.select([~draws, ~k_steps & has_step_kernel, ~k_steps, has_step_kernel & ~b["multi_split"]],
                     ["none", "fused", "two", "fused"], default="split")
    p = {"do_raster": draws, "fused": form == "fused", "split": form == "split"}
    p["frames"] = p["split"] & has_frame_kernel
    p["grouped"] = p["frames"] & b["env_grouped"]
    p["piped"] = p["grouped"] & b["pipe"] & b["all"]
    p["streamed"] = p["piped"] & b["stream"] & (i["streamed_rows"] >= 2) & b["st_words"]
    quarter = np.maximum(2, -(-i["nsteps"] // 4))
    steps = np.where(p["streamed"], np.minimum(i["nsteps"], i["streamed_rows"]),
                     np.where(p["piped"], np.minimum(i["chunk"], quarter), i["nsteps"]))
    ring_caps = ~p["fused"] & ~p["streamed"] & (i["ring_rows"] > 0)
    p["steps"] = np.where(ring_caps, np.minimum(steps, i["ring_rows"]), steps)
    return p


def test_plan_call_equals_its_restatement(calls):
    i, p = calls
    assert len(p["steps"]) == 2 ** 10 * len(CHUNKS) * len(KVARS) * len(NSTEPS) * len(RING_ROWS) * len(STREAMED_ROWS)
    want = restated_plan(i)
    for k in big_maps.CALL_PLAN:
        bad = np.flatnonzero(p[k] != want[k])
        assert not len(bad), (k, len(bad), {f: int(v[bad[0]]) for f, v in i.items()}, int(p[k][bad[0]]), int(want[k][bad[0]]))
    for k in big_maps.CALL_PLAN[:-1]:  # (every form occurs in the product)
        assert p[k].any() and not p[k].all(), k


def test_plan_call_invariants(calls):
    i, p = calls
    implies = lambda a, b: (~a | b).all()
    assert not (p["fused"] & p["split"]).any()
    assert implies(p["fused"] | p["split"], p["do_raster"])
    assert implies(p["streamed"], p["piped"]) and implies(p["piped"], p["frames"]) and implies(p["frames"], p["split"])
    assert implies(p["grouped"], p["frames"]) and implies(p["piped"], p["grouped"])
    assert implies(p["piped"], i["all"] != 0)
    packed = i["packed"] != 0
    assert not (packed & p["fused"]).any()
    assert implies(packed & (i["nsteps"] > 1) & p["do_raster"], p["split"])
    assert (p["steps"] >= 1).all() and (p["steps"] <= i["nsteps"]).all()
    assert implies(p["streamed"], p["steps"] <= i["streamed_rows"])
    assert implies(~p["fused"] & ~p["streamed"] & (i["ring_rows"] > 0), p["steps"] <= i["ring_rows"])


def kernel_name(p):
    """tc_env_launch_info's kernel names (no controller) from the plan's bits"""
    return np.select([p["fused"], p["grouped"], p["frames"], p["do_raster"]],
                     ["tc_step_kernel", "tc_envg_kernel+tc_frame_kernel", "tc_env_kernel+tc_frame_kernel", "tc_env_kernel+tc_raster_kernel"],
                     default="tc_env_kernel")


def test_plan_call_restatements_agree(calls):
    """the restatement above against the two the tests already had, on the inputs those cover: big_maps.expected_launch (a
    byte format that draws frames, TC_MULTI_SPLIT at its default: the kernel names by kvar, TC_FUSE and TC_ENV_GROUPED) and
    the chunk formula of test_gpu_call_sequences.check_launches (a piped chunked call whose ring holds a chunk)"""
    i, _ = calls
    want = restated_plan(i)
    names = kernel_name(want)
    covered = (i["multi_split"] == 1) & (i["packed"] == 0) & want["do_raster"]
    assert covered.any()
    for kvar in KVARS:
        for fuse in (0, 1):
            for grouped in (0, 1):
                for n in NSTEPS:
                    sel = covered & (i["kvar"] == kvar) & (i["fuse"] == fuse) & (i["env_grouped"] == grouped) & (i["nsteps"] == n)
                    _, name = big_maps.expected_launch({"kvar": kvar, "kframe": kvar}, n, fuse=bool(fuse), env_grouped=bool(grouped))
                    assert sel.any() and (names[sel] == name).all(), (kvar, fuse, grouped, n, name, set(names[sel]))
    chunked = want["piped"] & ~want["streamed"] & (i["ring_rows"] >= i["chunk"])
    assert chunked.any() and set(i["nsteps"][chunked]) == set(NSTEPS) - {1}
    k, chunk = i["nsteps"][chunked], i["chunk"][chunked]
    assert np.array_equal(want["steps"][chunked], np.minimum(chunk, np.maximum(2, (k + 3) // 4)))
