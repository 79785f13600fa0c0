"""The cull verdict that travels in a pose row (entry 13: tc_cull_row_encode / _decode / _verdict of
tinycarlo_amd/csrc/tc_cull.h), on the CPU: the helpers are built by the host compiler (tests/cull_row_shim.py) and the word
a pose-row writer stores for a pose is held against the reference, tc_cull_empty on that pose (tests/cull_shim.py).

The poses are every frame of an oracle rollout on simple_layout with bench.py's action distribution (v ~ U(0.3, 1),
s ~ U(-1, 1), a maneuver ~ U{0..3} held for 64 steps, auto-reset from a spawn queue): N_ENVS envs, STEPS steps behind a
pre-roll of PREROLL steps (cars start on the road, looking along it: it takes a while until some have left it).  Seed and
step counts are chosen so that the reference alone calls at least a tenth of these frames culled and at least a tenth
drawn; both shares are asserted, so a verdict that never says one of the two cannot pass."""
import subprocess

import numpy as np
import pytest

import cull_row_shim
import cull_shim
import orc
from common import setup

N_ENVS, PREROLL, STEPS, SEED = 64, 512, 32, 3
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return cull_row_shim.build_shim(tmp_path_factory.mktemp("tc_cull_row"))


def bench_rollout(m, car, cam, n=N_ENVS, preroll=PREROLL, steps=STEPS, seed=SEED):
    """-> poses [steps * n][3] = x, y, theta of every frame behind the pre-roll, draw-list lengths [steps * n]"""
    orc.set_math_mode(orc.MATH_PORTABLE)
    o = orc.Oracle(m, car, cam, orc.FMT_CLASSES, n, threads=4)
    rng = np.random.default_rng(seed)
    o.reset([m.sample_spawn_node(rng) for _ in range(n)], flags=orc.F_NO_OBSERVATION)
    o.spawn_queue = np.array([[m.sample_spawn_node(rng) for _ in range(64)] for _ in range(n)], dtype=np.int32)
    poses, nseg = [], []
    man = None
    for t in range(preroll + steps):
        if t % 64 == 0:
            man = rng.integers(0, 4, n).astype(np.int32)
        cc = np.stack([rng.uniform(0.3, 1, n), rng.uniform(-1, 1, n)], axis=1)
        o.step(cc, man, flags=orc.F_AUTORESET | orc.F_NO_OBSERVATION, with_obs=False)
        if t >= preroll:
            poses += [(o.state["x"][i], o.state["y"][i], o.state["theta"][i]) for i in range(n)]
            nseg += [len(o.segments(i)[0]) for i in range(n)]
    orc.set_math_mode(orc.MATH_LIBM)
    return np.array(poses), np.array(nseg)


@pytest.fixture(scope="module")
def frames():
    _, m, car, cam = setup("simple_layout", "r64")
    poses, nseg = bench_rollout(m, car, cam)
    poses.setflags(write=False)
    nseg.setflags(write=False)
    return m, cam, poses, nseg


def test_codec(shim):
    assert shim.row_entry() == 13
    draw, culled = shim.row_encode(0), shim.row_encode(1)
    assert (draw, culled) == (0, 1)
    assert ALL_ONES not in (np.uint64(draw), np.uint64(culled))  # never "not written yet"
    assert shim.row_decode(culled) == 1 and shim.row_decode(draw) == 0
    # whatever else the memory holds draws the frame (always right); only the one word skips it
    for w in (0xFFFFFFFFFFFFFFFF, 2, 1 << 32, 0x8000000000000001, 0x3FF0000000000000, 0x7FF8000000000000, 0xFFFFFFFF):
        assert shim.row_decode(w) == 0, hex(w)


def test_the_verdict_of_a_pose_is_the_predicate_on_that_pose(shim, frames):
    m, cam, poses, nseg = frames
    ref = cull_shim.Cull(shim, m, cam)
    assert ref.on and ref.nx > 0
    want = ref.empty(poses[:, 0], poses[:, 1], poses[:, 2])  # the reference: tc_cull_empty
    share = want.mean()
    print("simple_layout, %d envs, steps %d..%d, seed %d: %d frames, %.1f %% culled by the reference, %.1f %% without a segment"
          % (N_ENVS, PREROLL, PREROLL + STEPS, SEED, len(poses), 100 * share, 100 * (nseg == 0).mean()))
    assert share >= 0.10, share
    assert 1.0 - share >= 0.10, share
    w = cull_row_shim.verdicts(shim, ref, poses[:, 0], poses[:, 1], poses[:, 2])
    assert np.isin(w, np.array([shim.row_encode(0), shim.row_encode(1)], dtype=np.uint64)).all()
    assert not (w == ALL_ONES).any()
    got = np.array([shim.row_decode(int(x)) for x in w], dtype=bool)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert not (got & (nseg > 0)).any()  # (and no frame with a segment is skipped)


def test_cull_off_writes_draw(shim, frames):
    """a camera the derivation does not cover (H1: max_range below the longest edge) has no cover: every verdict is "draw" """
    m, _, poses, _ = frames
    _, _, _, cam = setup("simple_layout", "r64", max_range=0.05)
    ref = cull_shim.Cull(shim, m, cam)
    assert not ref.on
    w = cull_row_shim.verdicts(shim, ref, poses[:64, 0], poses[:64, 1], poses[:64, 2])
    assert (w == np.uint64(shim.row_encode(0))).all()


def test_standalone_program_under_sanitizers(tmp_path, frames):
    m, cam, poses, nseg = frames
    exe = cull_row_shim.build_program(tmp_path, sanitize=True)
    plain = cull_shim.build_shim(tmp_path)
    ref = cull_shim.Cull(plain, m, cam)
    want = ref.empty(poses[:, 0], poses[:, 1], poses[:, 2])
    inp = tmp_path / "poses.f64"
    ref.program_input(cam.K, int(cam.resolution[1]), int(cam.resolution[0]), float(cam.max_range), poses, nseg > 0).tofile(str(inp))
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.strip() == "culled %d of %d, wrong 0" % (int(want.sum()), len(poses)), r.stdout
