"""The host planners of tc_env_create (tinycarlo_amd/csrc/tc_plan.h) on the CPU: the header is built alone by the host
compiler (the shim of tests/big_maps.py) and the planners run on every bundled map, the stress map and the generated
maps of tests/big_maps.py (CASES: 320 .. 2 970 lane-line nodes, up to 16 layers, rings with gaps, dashes, interleaved and
duplicate edges, self-loops, isolated nodes; "<case>/<k>" below is map k of a case).

A plan that reports success is held to the properties the camera stage relies on ("Host structure"); whether
it must report failure is worked out here, independently, from the component sizes of the map.
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
