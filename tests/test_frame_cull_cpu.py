"""The whole-frame cull of tinycarlo_amd/csrc/tc_cull.h on the CPU: the header is built alone by the host compiler
(tests/cull_shim.py) and its predicate "this pose's draw list is empty" is held against the oracle's
orc_capture_segments.  The predicate may say "maybe" for an empty frame; it must never say "empty" for a frame with a
segment.

Every map runs with its own camera and with the same camera at max_range = 1 m: condition H1 of the header (every edge
shorter than max_range) switches the cull off for knuffingen, stress_graph and fuzz2007 at the bundled 0.5 m, and a
predicate that always answers "maybe" proves nothing.
"""
import subprocess

import numpy as np
import pytest

import cull_shim
import orc
from common import FUZZ_MAPS, GOLDEN, setup

MAPS = ["simple_layout", "knuffingen", "stress_graph"] + FUZZ_MAPS
RANGES = (None, 1.0)  # the config's own max_range, and 1 m


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cull_shim.build_shim(tmp_path_factory.mktemp("tc_cull"))


class Stage:
    def __init__(self, L, map_name, max_range=None):
        over = {} if max_range is None else {"max_range": max_range}
        _, self.m, self.car, self.cam = setup(map_name, "r64", **over)
        self.cull = cull_shim.Cull(L, self.m, self.cam)
        self.oracle = orc.Oracle(self.m, self.car, self.cam, orc.FMT_CLASSES, 1)

    def nseg(self, x, y, theta):
        st = self.oracle.state
        st["x"][0], st["y"][0], st["theta"][0] = x, y, theta
        return len(self.oracle.segments(0)[0])

    def check(self, poses, what):
        """no pose with a segment is called empty -> (poses culled, poses without a segment)"""
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        e = self.cull.empty(poses[:, 0], poses[:, 1], poses[:, 2])
        n = np.array([self.nseg(*p) for p in poses])
        bad = np.nonzero(e & (n > 0))[0]
        assert len(bad) == 0, (what, "called empty with segments:", [(poses[i].tolist(), int(n[i])) for i in bad[:5]])
        return int(e.sum()), int((n == 0).sum())


def rollout_poses(stage, n=8, steps=40, seed=0):
    """every frame of a short rollout with auto-reset and random actions"""
    orc.set_math_mode(orc.MATH_PORTABLE)
    o = orc.Oracle(stage.m, stage.car, stage.cam, orc.FMT_CLASSES, n)
    rng = np.random.default_rng(seed)
    o.reset([stage.m.sample_spawn_node(rng) for _ in range(n)], flags=orc.F_NO_OBSERVATION)
    o.spawn_queue = np.array([[stage.m.sample_spawn_node(rng) for _ in range(16)] for _ in range(n)], dtype=np.int32)
    out = []
    for _ in range(steps):
        cc = np.stack([rng.uniform(0.3, 1, n), rng.uniform(-1, 1, n)], axis=1)
        o.step(cc, rng.integers(0, 4, n).astype(np.int32), flags=orc.F_AUTORESET | orc.F_NO_OBSERVATION, with_obs=False)
        out += [(o.state["x"][i], o.state["y"][i], o.state["theta"][i]) for i in range(n)]
    return np.array(out)


def adversarial_poses(stage):
    return np.concatenate([cull_shim.boundary_poses(stage.cull), cull_shim.grid_poses(stage.cull)])


@pytest.mark.parametrize("map_name", MAPS)
def test_no_frame_with_a_segment_is_called_empty(shim, map_name):
    orc.set_math_mode(orc.MATH_PORTABLE)
    for mr in RANGES:
        st = Stage(shim, map_name, mr)
        steps = 20 if map_name == "knuffingen" else 40
        roll = rollout_poses(st, steps=steps)
        culled, empty = st.check(roll, "rollout")
        adv = adversarial_poses(st)
        a_culled, a_empty = st.check(adv, "adversarial") if len(adv) else (0, 0)
        print("%s max_range %s: cull %s (%d special nodes, longest edge %.3f m), rollout %d frames, %d empty, %d culled (%.1f %%); "
              "adversarial %d poses, %d empty, %d culled" % (map_name, st.cam.max_range, "on" if st.cull.on else "off", st.cull.n_special,
                                                            st.cull.lmax, len(roll), empty, culled, 100.0 * culled / len(roll), len(adv),
                                                            a_empty, a_culled))
        if st.cull.on:
            assert len(adv) > 0


def test_not_vacuous_on_simple_layout(shim):
    orc.set_math_mode(orc.MATH_PORTABLE)
    st = Stage(shim, "simple_layout")
    assert st.cull.on and st.cull.nx > 0
    outside = cull_shim.outside_poses(st.cull.nodes)
    lo, hi = st.cull.nodes.min(0), st.cull.nodes.max(0)
    assert all((p[0] < lo[0] - 2 or p[0] > hi[0] + 2 or p[1] < lo[1] - 2 or p[1] > hi[1] + 2) for p in outside)
    assert st.cull.empty(outside[:, 0], outside[:, 1], outside[:, 2]).all()
    road = cull_shim.road_poses(st.m)
    assert len(road) >= 8
    assert not st.cull.empty(road[:, 0], road[:, 1], road[:, 2]).any()
    assert all(st.nseg(*p) > 0 for p in road)  # (and they do see a line)
    st.check(outside, "outside")
    # both answers occur on the boundary ring, and with segments in view on its inner side
    ring = cull_shim.boundary_poses(st.cull)
    e = st.cull.empty(ring[:, 0], ring[:, 1], ring[:, 2])
    assert e.any() and not e.all()
    roll = rollout_poses(st, n=16, steps=400, seed=1)  # (long enough for cars to leave the road)
    culled, empty = st.check(roll, "rollout")
    print("simple_layout: %d rollout frames, %.1f %% empty, %.1f %% culled" % (len(roll), 100.0 * empty / len(roll), 100.0 * culled / len(roll)))
    assert culled > 0


def test_table_is_a_lower_bound(shim):
    """every cell's bound against brute-force distances from random points of the cell to every segment"""
    st = Stage(shim, "simple_layout")
    c = st.cull
    cells = c.cells()
    rng = np.random.default_rng(2)
    a, b = c.nodes[c.edges[:, 0]], c.nodes[c.edges[:, 1]]
    for _ in range(400):
        ix, iy = rng.integers(c.nx), rng.integers(c.ny)
        p = np.array([c.x0, c.y0]) + (np.array([ix, iy]) + rng.choice([0.0, 1.0, rng.uniform()], 2)) * c.cell
        ab = b - a
        t = np.clip(((p - a) * ab).sum(1) / np.maximum((ab * ab).sum(1), 1e-300), 0, 1)
        d = np.linalg.norm(p - (a + t[:, None] * ab), axis=1).min()
        assert cells[iy, ix] * c.cell <= d, (ix, iy, cells[iy, ix], d)
    assert cells.max() >= int(0.9 * c.margin / c.cell) and cells.min() == 0


def test_cover_contains_the_true_footprint(shim):
    """The 20 camera parameter sets of tests/golden/camera_sweep.*: every ground point that camera.py's E / K put in front,
    in range and strictly inside the image lies inside one of the cover's circles (numpy restatement, no tc_cull.h code)."""
    import json
    import os
    from tinycarlo_amd.camera import Camera
    with open(os.path.join(GOLDEN, "camera_sweep.json")) as f:
        sets = json.load(f)["sets"]
    assert len(sets) == 20
    _, m, _, _ = setup("simple_layout", "r64")
    gx, gy = np.meshgrid(np.arange(-1.5, 3.0, 0.004), np.arange(-2.5, 2.5, 0.004))
    pts = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size), np.ones(gx.size)])
    for s in sets:
        cam = Camera(dict(s))
        c = cull_shim.Cull(shim, m, cam)
        H, W = cam.resolution
        P = cam.E @ pts
        h = cam.K @ P
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = h[0] / h[2], h[1] / h[2]
        inside = (P[2] < 0) & (P[2] > -cam.max_range) & (u > 0) & (u < W) & (v > 0) & (v < H)
        assert c.on, s
        assert inside.sum() > 100, (s, int(inside.sum()))  # (the steepest set sees 0.005 m^2 of ground: ~300 samples)
        q = pts[:2, inside].T
        covered = np.zeros(len(q), dtype=bool)
        for (cx, cy, r) in c.circles:
            covered |= np.hypot(q[:, 0] - cx, q[:, 1] - cy) <= r
        assert covered.all(), (s, q[~covered][:3])
        # and the footprint polygon is not grossly larger than what the samples fill (a wrong sign would give the big square)
        area = 0.5 * abs(np.dot(c.poly[:, 0], np.roll(c.poly[:, 1], -1)) - np.dot(c.poly[:, 1], np.roll(c.poly[:, 0], -1)))
        assert inside.sum() * 0.004 ** 2 > 0.8 * area, (s, area, inside.sum() * 0.004 ** 2)


def test_planner_refuses_what_the_proof_excludes(shim):
    """H3 (a node with two in-edges whose in-neighbour has two out-edges), too many special nodes, H1 through the cover"""
    class G:
        def __init__(self, nodes, edges):
            self._f = {"node_count": np.array([len(nodes)], dtype=np.int32), "edge_count": np.array([len(edges)], dtype=np.int32),
                       "nodes": np.array(nodes, dtype=np.float64), "edges": np.array(edges, dtype=np.int32)}

        def flat(self):
            return self._f
    _, _, _, cam = setup("simple_layout", "r64")
    line = [[0.1 * i, 0.0] for i in range(6)]
    ok = cull_shim.Cull(shim, G(line, [[i, i + 1] for i in range(5)]), cam)
    assert ok.nx > 0 and ok.on and ok.n_special == 0
    fork = cull_shim.Cull(shim, G(line, [[0, 1], [1, 2], [1, 3], [3, 4]]), cam)  # node 1 has two out-edges
    assert fork.nx > 0 and fork.on and fork.n_special == 2
    diamond = cull_shim.Cull(shim, G(line, [[0, 1], [0, 2], [3, 2], [4, 5]]), cam)  # 1 <- 0 -> 2 <- 3
    assert diamond.nx == 0 and not diamond.on
    assert not diamond.empty(50.0, 50.0, 0.0)[0]
    long_edge = cull_shim.Cull(shim, G([[0, 0], [0.6, 0], [1.0, 0]], [[0, 1], [1, 2]]), cam)  # 0.6 m > max_range 0.5 m
    assert long_edge.nx > 0 and not long_edge.on
    assert not long_edge.empty(50.0, 50.0, 0.0)[0]
    assert ok.empty(50.0, 50.0, 0.0)[0]
    assert not ok.empty(np.nan, 0.0, 0.0)[0] and not ok.empty(0.0, 0.0, np.nan)[0] and not ok.empty(1e9, 0.0, 0.0)[0]


def test_sanitized_program_on_the_adversarial_set(shim, tmp_path):
    """tc_cull.h and the shim as a stand-alone program (its own main) under -fsanitize=address,undefined, run once over the
    adversarial poses of simple_layout with the oracle's answers beside them"""
    orc.set_math_mode(orc.MATH_PORTABLE)
    st = Stage(shim, "simple_layout")
    poses = np.concatenate([adversarial_poses(st), cull_shim.outside_poses(st.cull.nodes), cull_shim.road_poses(st.m)])
    nonempty = np.array([st.nseg(*p) > 0 for p in poses])
    exe = cull_shim.build_program(tmp_path)
    H, W = st.cam.resolution
    inp = tmp_path / "poses.f64"
    st.cull.program_input(st.cam.K, W, H, st.cam.max_range, poses, nonempty).astype(np.float64).tofile(str(inp))
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=120)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    expect = int(st.cull.empty(poses[:, 0], poses[:, 1], poses[:, 2]).sum())
    assert r.stdout.startswith("culled %d of %d, wrong 0" % (expect, len(poses))), r.stdout
