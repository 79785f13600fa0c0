"""Large random maps for the grouped and windowed camera paths, and the plan each of them must get.

Above 320 lane-line nodes or edges tc_env_create stops running the camera stage as one register-cached group
(plan_layers / plan_components / layout_lds in tinycarlo_hip.hip, tc_plan.h):

    max(nodes, edges) <= 320                                      K = 5, one group
    321 .. 512                                                    K = 8, one group
    > 512, largest layer <= 576, 2 .. 8 groups of whole layers    K = 9, layer groups
    ... and every connected component <= TC_CAM_GROUP, <= 8 groups, each an index range of the edge list
                                                                  component groups on a renumbered copy of the map;
                                                                  frame kernel 516 when the caps are <= 320, else K = 9
    otherwise                                                     K = 13, one group, windowed node / edge loops

`big_map` draws a map of given layer sizes and kinds whose lane lines hug the lane path, so that cars see them;
`expected_plan` works out the row of the table above from tc_plan.h itself (built alone by the host compiler) and a
restatement of the three decisions around it; `CASES` names one seeded map per boundary and branch.
tests/test_big_maps_cpu.py holds every case to its name and to frames that are worth comparing;
tests/test_gpu_big_map_fuzz.py runs them on the GPU against the oracle.  Test infrastructure only.
"""
import atexit
import copy
import ctypes as C
import math
import os
import shutil
import subprocess
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NT = 64            # TC_NT
MAX_GROUPS = 8     # TC_MAX_GROUPS
MAX_LAYERS = 16    # TC_MAX_LAYERS
CAM_GROUP = 5 * NT  # default of TC_CAM_GROUP
LAYER_CAP = 9 * NT  # the K = 9 register cache: largest layer of the layer scheme
LDS_LIMIT = 160 * 1024
LIVE_BYTES = 416   # TC_LIVE_BYTES: the parked env state behind both stages' buffers

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
struct Lds {
  int off_p, off_flg, off_list, off_cnt, total;
};
// out: off_p, off_flg, off_list, off_cnt, total
extern "C" void cam_lds(int cap_n, int cap_e, int total_nodes, int* out) {
  Lds L;
  plan_cam_lds(L, cap_n, cap_e, total_nodes);
  const int v[5] = {L.off_p, L.off_flg, L.off_list, L.off_cnt, L.total};
  std::copy(v, v + 5, out);
}
// in: n rows of 16 ints, the fields of CallInputs in their order; out: n rows of 8, the fields of CallPlan in theirs
extern "C" void plan_calls(const int* in, int n, int* out) {
  for (int i = 0; i < n; i++, in += 16, out += 8) {
    CallInputs c;
    c.fuse = in[0], c.multi_split = in[1], c.env_grouped = in[2], c.pipe = in[3], c.stream = in[4], c.chunk = in[5];
    c.kvar = in[6], c.packed = in[7] != 0, c.ring_rows = in[8], c.streamed_rows = in[9], c.st_words = in[10] != 0;
    c.flags = (unsigned)in[11], c.no_frame_flags = (unsigned)in[12], c.nsteps = in[13], c.obs = in[14] != 0, c.all = in[15] != 0;
    const CallPlan p = plan_call(c);
    const int v[8] = {p.do_raster, p.fused, p.split, p.frames, p.grouped, p.piped, p.streamed, p.steps};
    std::copy(v, v + 8, out);
  }
}
"""
CALL_INPUTS = ("fuse", "multi_split", "env_grouped", "pipe", "stream", "chunk", "kvar", "packed", "ring_rows", "streamed_rows",
               "st_words", "flags", "no_frame_flags", "nsteps", "obs", "all")
CALL_PLAN = ("do_raster", "fused", "split", "frames", "grouped", "piped", "streamed", "steps")


def plan_calls(lib, rows):
    """plan_call through the shim over many inputs: rows [n, len(CALL_INPUTS)] int32 -> [n, len(CALL_PLAN)] int32"""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    assert rows.ndim == 2 and rows.shape[1] == len(CALL_INPUTS)
    out = np.zeros((len(rows), len(CALL_PLAN)), dtype=np.int32)
    lib.plan_calls(_ptr(rows), len(rows), _ptr(out))
    return out


def build_plan_shim(d):
    """-> ctypes library of tc_plan.h built alone by the host compiler in directory d"""
    src, lib = os.path.join(str(d), "shim.cpp"), os.path.join(str(d), "libtc_plan.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"), "-o", lib, src])
    return C.CDLL(lib)


_lib = None


def plan_lib():
    """the shim, built once per process in a directory of its own"""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="tc_plan_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        _lib = build_plan_shim(d)
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def graph_arrays(node_count, edge_count, edges_local):
    """-> (node_off, edge_off, edges with global node ids) as int32 arrays"""
    node_off = np.concatenate([[0], np.cumsum(node_count)]).astype(np.int32)
    edge_off = np.concatenate([[0], np.cumsum(edge_count)]).astype(np.int32)
    e = np.asarray(edges_local, dtype=np.int64).reshape(-1, 2)
    edges = np.ascontiguousarray(e + np.repeat(node_off[:-1], edge_count)[:, None], dtype=np.int32)
    return node_off, edge_off, edges


def graph_of_json(mj):
    ls = list(mj["lanelines"].values())
    return graph_arrays([len(l["nodes"]) for l in ls], [len(l["edges"]) for l in ls], [e for l in ls for e in l["edges"]])


# ---------------------------------------------------------------------------------------------- the generator
def _ellipse(geo, a, s=1.0):
    return geo["cx"] + s * geo["rx"] * math.cos(a), geo["cy"] + s * geo["ry"] * math.sin(a)


def _lanepath(rng, geo):
    """a two-way ring of about 60 nodes on the ellipse, with a few of random_map's chords, a hub and a dead end"""
    n = int(rng.integers(54, 67))
    ang = np.sort(rng.uniform(0, 2 * math.pi, n))
    nodes = [[int(x + rng.normal(0, 3)), int(y + rng.normal(0, 3))] for x, y in (_ellipse(geo, a) for a in ang)]
    edges = [[i, (i + 1) % n] for i in range(n)] + [[(i + 1) % n, i] for i in range(n)]
    for _ in range(int(rng.integers(0, 3))):     # chords (may be a self-loop)
        a, b = rng.integers(0, n, 2)
        edges.append([int(a), int(b)])
    if rng.random() < 0.4:                       # a hub with several successors / predecessors
        hub = len(nodes)
        a = rng.uniform(0, 2 * math.pi)
        x, y = _ellipse(geo, a, 0.8)
        nodes.append([int(x), int(y)])
        for k in rng.choice(n, size=int(rng.integers(2, 6)), replace=False):
            edges.append([hub, int(k)])
        for k in rng.choice(n, size=int(rng.integers(1, 4)), replace=False):
            edges.append([int(k), hub])
    if rng.random() < 0.5:                       # dead end
        d = len(nodes)
        nodes.append([int(geo["cx"] + geo["rx"] + 40), int(geo["cy"])])
        edges.append([0, d])
    if rng.random() < 0.5:
        edges.append(list(edges[int(rng.integers(0, len(edges)))]))   # duplicate edge
    return {"layer_color": [255, 255, 255], "nodes": nodes, "edges": edges}


def _ring_nodes(rng, geo, n, a0, span):
    s = rng.uniform(0.9, 1.1)
    closed = span >= 2 * math.pi
    step = span / (n if closed else max(n - 1, 1))
    return [[int(x + rng.normal(0, 0.7)), int(y + rng.normal(0, 0.7))] for x, y in (_ellipse(geo, a0 + step * i, s) for i in range(n))]


def _drop(rng, edges, gaps):
    """the edge list without `gaps` of its edges (None: about 3 %, at least one)"""
    k = max(1, round(0.03 * len(edges))) if gaps is None else int(gaps)
    gone = set(rng.choice(len(edges), size=min(k, len(edges)), replace=False).tolist()) if k else set()
    return [e for i, e in enumerate(edges) if i not in gone]


def _layer(rng, geo, n, kind, opts):
    gaps = opts.get("gaps")
    if kind in ("ring", "doubled"):      # a polyline all the way round, some edges missing: components of mixed size
        nodes = _ring_nodes(rng, geo, n, rng.uniform(0, 2 * math.pi), 2 * math.pi)
        edges = _drop(rng, [[i, (i + 1) % n] for i in range(n)], gaps)
        if kind == "doubled":            # every edge twice, so that edges exceed nodes: side by side, or the list repeated
            edges = [e for e in edges for _ in range(2)] if rng.random() < 0.5 else edges + [list(e) for e in edges]
    elif kind == "half":                 # a polyline over the map's half of the ellipse only (rather more than half of it:
                                         # a car sees the lines from up to max_range outside)
        nodes = _ring_nodes(rng, geo, n, geo["half0"] + rng.uniform(0, 0.1), math.pi * rng.uniform(1.15, 1.3))
        edges = _drop(rng, [[i, i + 1] for i in range(n - 1)], gaps)
    elif kind == "dashes":               # node pairs, centres on the ellipse +- 30 px; an odd node is left over
        ang = rng.uniform(0, 2 * math.pi, n // 2)
        if rng.random() < 0.5:
            ang = np.sort(ang)
        nodes = []
        for a in ang:
            x, y = _ellipse(geo, a)
            x, y = int(x + rng.uniform(-30, 30)), int(y + rng.uniform(-30, 30))
            nodes += [[x, y], [x + int(rng.integers(-25, 26)), y + int(rng.integers(-25, 26))]]
        edges = [[i, i + 1] for i in range(0, n - 1, 2)]
        if n % 2:
            nodes.append([int(v) for v in _ellipse(geo, rng.uniform(0, 2 * math.pi))])
    elif kind == "mess":                 # blocks of four nodes: interleaved edges, a self-loop, a duplicate, an isolated node
        nodes, edges = [], []
        for b in range(n // 4):
            i = 4 * b
            x, y = _ellipse(geo, rng.uniform(0, 2 * math.pi))
            x, y = x + rng.uniform(-30, 30), y + rng.uniform(-30, 30)
            blk = [[int(x + rng.integers(-20, 21)), int(y + rng.integers(-20, 21))] for _ in range(4)]
            first = rng.random() < 0.5
            if rng.random() < 0.1:       # a zero-length edge: two nodes at the same pixel
                blk[1 if first else 2] = list(blk[0])
            nodes += blk
            edges += [[i, i + 1], [i + 2, i + 3], [i + 1, i + 2]] if first else [[i, i + 2], [i + 1, i + 1], [i, i + 2]]
        for _ in range(n % 4):
            nodes.append([int(v) for v in _ellipse(geo, rng.uniform(0, 2 * math.pi))])
    else:
        raise KeyError(kind)
    assert len(nodes) == n
    return {"layer_color": [int(v) for v in rng.integers(0, 256, 3)], "nodes": nodes, "edges": edges}


def big_map(rng, layers, W=1200, H=800):
    """A map in the reference's JSON schema.  layers: [(n_nodes, kind)] or [(n_nodes, kind, {"gaps": edges removed})],
    kind one of ring / dashes / mess / doubled / half; every layer hugs the ellipse of the lane path."""
    geo = {"cx": W / 2, "cy": H / 2, "rx": rng.uniform(400, 480), "ry": rng.uniform(260, 320), "half0": rng.uniform(0, 2 * math.pi)}
    lanepath = _lanepath(rng, geo)
    lanes = {}
    for li, spec in enumerate(layers):
        lanes[f"{spec[1]}{li}"] = _layer(rng, geo, int(spec[0]), spec[1], spec[2] if len(spec) > 2 else {})
    return {"width": W, "height": H, "lanelines": lanes, "lanepath": lanepath}


# ---------------------------------------------------------------------------------------------- the plan
def cam_lds(cap_n, cap_e, total_nodes):
    """plan_cam_lds through the shim -> {off_p, off_flg, off_list, off_cnt, total}"""
    out = np.zeros(5, dtype=np.int32)
    plan_lib().cam_lds(int(cap_n), int(cap_e), int(total_nodes), _ptr(out))
    return dict(zip(("off_p", "off_flg", "off_list", "off_cnt", "total"), (int(v) for v in out)))


def expected_plan(map_json, cam_group=CAM_GROUP, groups=True):
    """The plan a handle on this map must get: the planners of tc_plan.h through the shim, and the three decisions of
    plan_layers, plan_components and layout_lds restated with the thresholds of the table at the head of this file.
    -> kvar, n_groups, scheme (single | layers | components), cap_n, cap_e, kframe; the groups' bounds n0, e0 (nodes /
    edges, in the camera copy's numbering for component groups) and l0, l1 (layers l0[g] .. l1[g] - 1); total_nodes,
    total_edges, n_layers and the camera stage's LDS layout (lds)."""
    node_off, edge_off, edges = graph_of_json(map_json)
    nl, tn, te = len(node_off) - 1, int(node_off[-1]), int(edge_off[-1])
    big = max(tn, te)
    p = {"kvar": 5 if big <= 5 * NT else 8 if big <= 8 * NT else 13, "n_groups": 1, "scheme": "single", "cap_n": tn, "cap_e": te,
         "n0": [0, tn], "e0": [0, te], "l0": [0], "l1": [nl]}
    L = plan_lib()
    caps = np.zeros(2, dtype=np.int32)
    if big > 8 * NT and groups:
        layer = np.zeros(MAX_GROUPS + 1, dtype=np.int32)
        ng = L.layers(_ptr(node_off), _ptr(edge_off), nl, LAYER_CAP, MAX_GROUPS, _ptr(layer), _ptr(caps))
        if ng:
            layer = layer[:ng + 1]
            p.update(kvar=9, n_groups=ng, scheme="layers", cap_n=int(caps[0]), cap_e=int(caps[1]), n0=node_off[layer].tolist(),
                     e0=edge_off[layer].tolist(), l0=layer[:-1].tolist(), l1=layer[1:].tolist())
    if p["scheme"] == "layers" and NT <= cam_group <= LAYER_CAP:
        new_id = np.zeros(max(tn, 1), dtype=np.int32)
        n0, e0 = np.zeros(MAX_GROUPS + 1, dtype=np.int32), np.zeros(MAX_GROUPS + 1, dtype=np.int32)
        l0, l1 = np.zeros(MAX_GROUPS, dtype=np.int32), np.zeros(MAX_GROUPS, dtype=np.int32)
        ng = L.components(_ptr(edge_off), nl, _ptr(edges), tn, int(cam_group), MAX_GROUPS, _ptr(new_id), _ptr(n0), _ptr(e0), _ptr(l0),
                          _ptr(l1), _ptr(caps))
        if ng:
            p.update(n_groups=ng, scheme="components", cap_n=int(caps[0]), cap_e=int(caps[1]), n0=n0[:ng + 1].tolist(),
                     e0=e0[:ng + 1].tolist(), l0=l0[:ng].tolist(), l1=l1[:ng].tolist())
    small = p["cap_n"] <= 5 * NT and p["cap_e"] <= 5 * NT
    p["kframe"] = 516 if p["scheme"] == "components" and small else p["kvar"]
    p.update(total_nodes=tn, total_edges=te, n_layers=nl, lds=cam_lds(p["cap_n"], p["cap_e"], tn))
    return p


def expected_launch(plan, n_steps, fuse=True, env_grouped=True):
    """(kvar, kernel) that launch_info(n_steps) must report for a handle of this plan that draws frames (plan_call)"""
    can_fuse = fuse and plan["kvar"] != 13   # (the K = 13 simulate stage stays two launches)
    if n_steps == 1:
        if can_fuse:
            return (5 if plan["kframe"] == 516 else plan["kvar"]), "tc_step_kernel"
        return plan["kvar"], "tc_env_kernel+tc_raster_kernel"
    if can_fuse:
        return plan["kvar"], ("tc_envg_kernel" if env_grouped else "tc_env_kernel") + "+tc_frame_kernel"
    return plan["kvar"], "tc_env_kernel+tc_raster_kernel"


def split_layers(plan):
    """layers whose edges are shared between two groups"""
    return [plan["l0"][g + 1] for g in range(plan["n_groups"] - 1) if plan["l0"][g + 1] < plan["l1"][g]]


def spanning_groups(plan):
    """groups that hold edges of two layers or more"""
    return [g for g in range(plan["n_groups"]) if plan["l1"][g] - plan["l0"][g] >= 2]


# ---------------------------------------------------------------------------------------------- the cases
def _c(layers, want, **kw):
    d = {"layers": layers, "want": want, "cam_group": CAM_GROUP, "fmt": "classes", "res": [64, 64], "ppm": 300}
    d.update(kw)
    return d


K5 = {"scheme": "single", "kvar": 5, "kframe": 5}
K8 = {"scheme": "single", "kvar": 8, "kframe": 8}
K13 = {"scheme": "single", "kvar": 13, "kframe": 13}
LAYERS = {"scheme": "layers", "kvar": 9, "kframe": 9}
COMP516 = {"scheme": "components", "kvar": 9, "kframe": 516}
COMP9 = {"scheme": "components", "kvar": 9, "kframe": 9}
R, D, M, DB, HF = "ring", "dashes", "mess", "doubled", "half"

# `want` holds what expected_plan must return; split / span: a layer split between two groups / a group of several
# layers must be in the plan; why: the reason the component planner must refuse (test_plan_cpu._expect_failure's words);
# windows: (node windows, edge windows) of the K = 13 loops.  A map that misses its `want` is drawn again (case_map).
CASES = {
    "k5_320_nodes": _c([(200, R), (120, D)], dict(K5, total_nodes=320)),
    "k8_321_nodes": _c([(200, R), (121, R)], dict(K8, total_nodes=321), fmt="rgb"),
    "k8_by_edges": _c([(100, DB), (110, DB), (60, D)], dict(K8, max_nodes=320, min_edges=321)),
    "k8_512_nodes": _c([(256, R), (156, M), (100, D)], dict(K8, total_nodes=512), res=[48, 80]),
    "groups_513_nodes": _c([(257, R), (156, M), (100, D)], dict(scheme=("layers", "components"), kvar=9, total_nodes=513)),
    "components_516_split": _c([(300, R), (300, D), (200, D), (12, R)], dict(COMP516, split=True, span=True)),
    "components_mess": _c([(300, M), (300, M)], dict(COMP516, split=True)),
    "components_cap_576": _c([(500, R), (400, D)], dict(COMP9, min_cap=321), cam_group=576, ppm=200),
    "components_16_layers": _c([(560, D)] + [(36 + (i % 3), (D, M, R)[i % 3]) for i in range(15)], dict(COMP516, span=True, n_layers=16)),
    "components_half": _c([(300, HF), (300, HF), (200, HF)], dict(COMP516, cull=True, empty_frac=0.1)),
    "layers_big_component": _c([(400, R, {"gaps": 0}), (300, D)], dict(LAYERS, why="component larger than T")),
    "layers_cap_576": _c([(576, R, {"gaps": 0}), (300, D), (200, M)], dict(LAYERS, cap=576, why="component larger than T"), fmt="rgb"),
    "layers_too_many_components": _c([(330, (R, D)[i % 2]) for i in range(8)], dict(LAYERS, why="too many groups", n_groups=8)),
    "layers_interleaved_border": _c([(200, D), (400, M), (200, R)], dict(LAYERS, why="groups are not ranges of the edge list")),
    "k13_layer_577": _c([(577, R), (200, D)], dict(K13, windows=(1, 1))),
    "k13_one_layer_700": _c([(700, D)], dict(K13, windows=(1, 1)), ppm=200),
    "k13_by_edges": _c([(600, DB)], dict(K13, windows=(1, 2), max_nodes=832, min_edges=833)),
    "k13_9_layers_2970": _c([(330, (R, D, M)[i % 3]) for i in range(9)], dict(K13, windows=(4, None), total_nodes=2970, min_lds=48 * 1024)),
}
SWITCH_CASES = ("components_516_split", "layers_cap_576", "k13_by_edges")
N_ENVS, N_STEPS = 64, 12   # envs; single steps, and steps of the one K-step call behind them
N_SEEDS = int(os.environ.get("TC_BIG_FUZZ_SEEDS", "1"))


def plan_misses(plan, want):
    """what keeps `plan` from being the plan the case is named for ([] = nothing)"""
    bad = []
    for k in ("scheme", "kvar", "kframe", "total_nodes", "n_layers", "n_groups"):
        if k in want and not (plan[k] in want[k] if isinstance(want[k], tuple) else plan[k] == want[k]):
            bad.append((k, plan[k], want[k]))
    big = max(plan["cap_n"], plan["cap_e"])
    if "cap" in want and big != want["cap"]:
        bad.append(("cap", big, want["cap"]))
    if "min_cap" in want and big < want["min_cap"]:
        bad.append(("min_cap", big, want["min_cap"]))
    if "max_nodes" in want and plan["total_nodes"] > want["max_nodes"]:
        bad.append(("max_nodes", plan["total_nodes"]))
    if "min_edges" in want and plan["total_edges"] < want["min_edges"]:
        bad.append(("min_edges", plan["total_edges"]))
    if want.get("split") and not split_layers(plan):
        bad.append("no layer is split between two groups")
    if want.get("span") and not spanning_groups(plan):
        bad.append("no group spans two layers")
    if "windows" in want:
        w = (-(-plan["cap_n"] // (13 * NT)), -(-plan["cap_e"] // (13 * NT)))
        if any(x is not None and x != y for x, y in zip(want["windows"], w)):
            bad.append(("windows", w, want["windows"]))
    if "min_lds" in want and plan["lds"]["total"] <= want["min_lds"]:
        bad.append(("min_lds", plan["lds"]["total"]))
    if plan["total_nodes"] >= 3000 or plan["n_layers"] > MAX_LAYERS:
        bad.append("map too large")
    return bad


def case_rng(name, k, stream):
    return np.random.default_rng([zlib.crc32(name.encode()), int(k), int(stream)])


_maps = {}


def case_map(name, k=0):
    """map `k` of a case: maps are drawn from the case's seeded stream until one gets the plan the case is named for
    (where a group border falls depends on where the generator left its gaps) -> (map_json, plan)"""
    if (name, k) not in _maps:
        case = CASES[name]
        rng = case_rng(name, k, 0)
        for _ in range(64):
            mj = big_map(rng, case["layers"])
            plan = expected_plan(mj, cam_group=case["cam_group"])
            if not plan_misses(plan, case["want"]):
                break
        else:
            raise AssertionError((name, k, "no map of these layers gets the plan", plan_misses(plan, case["want"])))
        _maps[(name, k)] = (mj, plan)
    mj, plan = _maps[(name, k)]
    return copy.deepcopy(mj), plan


def case_config(name, k, json_path):
    """the config of map `k` of a case, its map written to json_path: simple_layout's car and camera at the case's
    resolution and format, line thickness drawn from 1 .. 4"""
    import json
    from common import load_cfg
    case = CASES[name]
    with open(json_path, "w") as f:
        json.dump(case_map(name, k)[0], f)
    cfg = copy.deepcopy(load_cfg("simple_layout")[0])
    cfg["map"] = {"json_path": str(json_path), "pixel_per_meter": case["ppm"]}
    cfg["sim"]["observation_space_format"] = case["fmt"]
    cfg["camera"].update(resolution=list(case["res"]), line_thickness=int(case_rng(name, k, 1).integers(1, 5)))
    return cfg


def case_actions(name, k, n=N_ENVS, steps=2 * N_STEPS):
    """wild controls (beyond [-1, 1]) and all four maneuvers -> (car_control [steps][n][2] f32, maneuver [steps][n] i32)"""
    rng = case_rng(name, k, 2)
    cc = np.stack([rng.uniform(-0.6, 1.3, (steps, n)), rng.uniform(-1.3, 1.3, (steps, n))], axis=2).astype(np.float32)
    return cc, rng.integers(0, 4, (steps, n)).astype(np.int32)


def case_seed(name, k):
    """seed of the env's reset (spawn nodes and spawn queue)"""
    return int(case_rng(name, k, 3).integers(0, 1 << 30))
