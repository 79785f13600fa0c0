"""The host planners of tc_env_create (tinycarlo_amd/csrc/tc_plan.h) on the CPU: the header is built alone by the host
compiler and the planners run on every bundled map and the stress map.

A plan that reports success is held to the properties the camera stage relies on ("Host structure"); whether
it must report failure is worked out here, independently, from the component sizes of the map.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from common import ROOT, setup

MAX_GROUPS = 8   # TC_MAX_GROUPS
NT = 64          # TC_NT
MAPS = ["simple_layout", "knuffingen", "formula_student_track", "stress_graph"]

SHIM = r"""
#include "tc_plan.h"
#include <algorithm>
extern "C" int components(const int* edge_off, int C, const int* edges, int n_nodes, int T, int max_groups, int* new_id,
                          int* n0, int* e0, int* l0, int* l1, int* caps) {
  const ComponentGroups p = plan_component_groups(edge_off, C, edges, n_nodes, T, max_groups);
  if (!p.ok) return 0;
  std::copy(p.new_id.begin(), p.new_id.end(), new_id);
  std::copy(p.n0.begin(), p.n0.end(), n0);
  std::copy(p.e0.begin(), p.e0.end(), e0);
  std::copy(p.l0.begin(), p.l0.end(), l0);
  std::copy(p.l1.begin(), p.l1.end(), l1);
  caps[0] = p.cap_n;
  caps[1] = p.cap_e;
  return (int)p.l0.size();
}
extern "C" int layers(const int* node_off, const int* edge_off, int C, int max_cap, int max_groups, int* layer, int* caps) {
  const LayerGroups p = plan_layer_groups(node_off, edge_off, C, max_cap, max_groups);
  if (!p.ok) return 0;
  std::copy(p.layer.begin(), p.layer.end(), layer);
  caps[0] = p.cap_n;
  caps[1] = p.cap_e;
  return (int)p.layer.size() - 1;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("tc_plan")
    src, lib = d / "shim.cpp", d / "libtc_plan.so"
    src.write_text(SHIM)
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"), "-o", str(lib), str(src)])
    return C.CDLL(str(lib))


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.fixture(scope="module")
def graphs():
    """map name -> (node_off, edge_off, edges with global node ids, component label of every node, -1 = no edge)"""
    out = {}
    for name in MAPS:
        f = setup(name)[1].flat()
        node_off = np.concatenate([[0], np.cumsum(f["node_count"])]).astype(np.int32)
        edge_off = np.concatenate([[0], np.cumsum(f["edge_count"])]).astype(np.int32)
        edges = np.ascontiguousarray(f["edges"] + np.repeat(node_off[:-1], f["edge_count"])[:, None], dtype=np.int32)
        label = np.arange(node_off[-1])
        while True:  # label propagation: every node takes the smallest id its edges reach
            lo = np.minimum(label[edges[:, 0]], label[edges[:, 1]])
            new = label.copy()
            np.minimum.at(new, edges[:, 0], lo)
            np.minimum.at(new, edges[:, 1], lo)
            if np.array_equal(new, label):
                break
            label = new
        has_edge = np.zeros(node_off[-1], dtype=bool)
        has_edge[edges.ravel()] = True
        out[name] = (node_off, edge_off, edges, np.where(has_edge, label, -1))
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


@pytest.mark.parametrize("T", [320, 200, 64])
@pytest.mark.parametrize("name", MAPS)
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
