"""CPU companions of tests/test_gpu_variant_matrix.py: what the matrix relies on, checked without a GPU.

  * the expected instantiation set against the kernel symbols of the built library, one to one;
  * the matrix's parametrisation against that set: every instantiation has a case that is there to launch it;
  * every case's reference run (tests/feature_ref.py alone) meets the conditions under which the case tests something, so
    the GPU run is never the first to learn that a case is vacuous;
  * every column of the per-env car rows changes the reference's result on the cases' inputs (a kernel that read the shared
    car's constant instead would be caught);
  * the composed reference with every layer off is the plain batched oracle, bit for bit;
  * its episode layer equals the `Ref` of tests/test_gpu_episodes.py on that file's simple_layout inputs."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import feature_ref as fr
import orc
import test_gpu_variant_matrix as vm
from common import ROOT

LIB = os.path.join(ROOT, "tinycarlo_amd", "libtinycarlo_hip.so")
FMT_NAME = {0: "rgb", 1: "classes", 2: "bits"}  # TC_FMT_RGB, TC_FMT_CLASSES, TC_FMT_CLASSES_BITS
FAMILIES = ("step", "drive_step", "env", "drive_env", "envg", "drive_envg", "frame", "frame_recover", "raster")


@pytest.fixture(autouse=True)
def _portable():
    orc.set_math_mode(orc.MATH_PORTABLE)
    yield
    orc.set_math_mode(orc.MATH_LIBM)


def kcode_of(K, RB):
    """the code of a (K, RB) pair (StepKRb of tinycarlo_hip.hip): K 5 with batches of 16 is 516, else K with RB_OF_K(K)"""
    if (K, RB) == (5, 16):
        return 516
    assert RB == (16 if K >= 8 else 32), (K, RB)
    return K


def kernel_entry(name):
    """ledger entry (family, K or kcode, THICK or CAM, FMT, FEAT) of a kernel's mangled name, None for other symbols --
    common.kernel_variant extended to the tc_drive_*, frame, recover and raster names:
    _Z20tc_drive_step_kernelILi5ELb1ELi1ELi16ELj7EEv8StepArgs is tc_drive_step_kernel<5, true, TC_FMT_CLASSES, 16, 7u>"""
    m = re.match(r"_Z\d+tc_(\w+?)_kernelI((?:L[ibj]\d+E)+)Ev\d+(?:StepArgs|FrameArgs|RArgs)$", name)
    if not m or m.group(1) not in FAMILIES:
        return None
    fam = m.group(1)
    a = [int(v) for v in re.findall(r"L[ibj](\d+)E", m.group(2))]
    if fam in ("step", "drive_step"):
        K, T, F, RB, feat = a
        return (fam, kcode_of(K, RB), bool(T), FMT_NAME[F], feat)
    if fam in ("env", "drive_env"):
        K, cam, feat = a
        return (fam, K, bool(cam), None, feat)
    if fam in ("envg", "drive_envg"):
        return (fam, None, None, None, a[0])
    if fam in ("frame", "frame_recover"):
        K, T, F, RB = a
        return (fam, kcode_of(K, RB), bool(T), FMT_NAME[F], None)
    T, F = a
    return (fam, None, bool(T), FMT_NAME[F], None)


def test_expected_set_equals_the_librarys_kernel_symbols():
    """`nm -D` on the built library: the dynamic table holds one object per kernel (its handle) and one __device_stub__
    function, both under the kernel's mangled name.  Symbol names only: no kernel code is read."""
    assert os.path.exists(LIB), "build the library first (__graft_entry__.build)"
    nm = shutil.which("nm") or "/opt/rocm/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", LIB], check=True, capture_output=True, text=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    kernels = [n for n in names if re.match(r"_Z\d+tc_\w+_kernel", n) and "__device_stub__" not in n]
    of_family = [n for n in kernels if re.match(r"_Z\d+tc_(%s)_kernelI" % "|".join(FAMILIES), n)]
    entries = {}
    for n in of_family:
        e = kernel_entry(n)
        assert e is not None, ("a kernel symbol of the five families that the parser does not read", n)
        assert e not in entries, ("two symbols for one entry", n, entries[e])
        entries[e] = n
    # (the other kernels of the library have no template variants to cover: gate, noise, order, unpack)
    others = {re.match(r"_Z\d+(tc_\w+?_kernel)", n).group(1) for n in kernels if n not in of_family}
    assert others <= {"tc_gate_kernel", "tc_noise_kernel", "tc_noise_tick", "tc_order_kernel", "tc_unpack_bits_kernel"}, others
    got = set(entries)
    assert got - vm.EXPECTED == set(), ("compiled but not in the matrix", sorted(got - vm.EXPECTED, key=str))
    assert vm.EXPECTED - got == set(), ("in the matrix but not compiled", sorted(vm.EXPECTED - got, key=str))
    print(f"\nvariant matrix: {len(got)} kernel instantiations in the symbol table")
    assert len(got) == len(vm.EXPECTED) == 254
    by_family = {f: sum(1 for e in got if e[0] == f) for f in FAMILIES}
    assert by_family == {"step": 64, "drive_step": 64, "env": 32, "drive_env": 32, "envg": 4, "drive_envg": 4, "frame": 24,
                         "frame_recover": 24, "raster": 6}


def test_parametrisation_covers_the_expected_set():
    planned = set()
    for part, cases in (("A", vm.PART_A), ("B", vm.PART_B), ("C", vm.PART_C)):
        assert len(set(cases)) == len(cases)
        for c in cases:
            planned |= vm.planned_entries(part, c)
    assert planned == vm.EXPECTED, (sorted(vm.EXPECTED - planned, key=str), sorted(planned - vm.EXPECTED, key=str))
    assert (len(vm.PART_A), len(vm.PART_B), len(vm.PART_C)) == (128, 32, 24)
    # a case asserts its plan against big_maps.expected_launch: the maps must have the plans the K codes stand for
    for kc in (5, 8, 9, 516, 13):
        plan = fr.case_plan(kc)
        assert plan["kframe"] == kc and plan["kvar"] == (9 if kc == 516 else kc), (kc, plan["kvar"], plan["kframe"])


def reference_cells():
    """the (kcode, thick, fmt, feat) reference runs the three parts use"""
    cells = set(vm.PART_A)
    cells |= {(k, True, "classes", ft) for k, ft in vm.PART_B}
    cells |= {(kc, t, "rgb" if f == "rgb" else "classes", 0) for kc, t, f in vm.PART_C}
    return sorted(cells, key=str)


@pytest.mark.parametrize("kcode", (5, 516, 8, 9, 13))
def test_no_case_is_vacuous_on_the_reference_alone(kcode):
    cells = [c for c in reference_cells() if c[0] == kcode]
    assert len(cells) == (8 if kcode == 13 else 32)
    for kc, thick, fmt, feat in cells:
        run = fr.reference_run(kc, thick, fmt, feat)
        fr.assert_not_vacuous(run, feat, (kc, thick, fmt, feat))
        if fmt == "classes":  # packed frames are these with 8 pixels per byte: the width must allow it
            assert fr.RES[1] % 32 == 0
        # what the recover pass of part C is left with ((row + env) % 3 == 0) is not all empty
        left = (np.arange(fr.N_MULTI)[:, None] + np.arange(fr.N_ENVS)[None, :]) % 3 == 0
        assert np.stack([s["obs"] for s in run["steps"][fr.N_SINGLE:]])[left].any()


@pytest.mark.parametrize("feat", (fr.FEAT_CAR, fr.FEAT_CAR | fr.FEAT_CTRL))
@pytest.mark.parametrize("kcode", (5, 516, 8, 9, 13))
def test_every_car_column_makes_a_difference(kcode, feat):
    """The inputs let every column of an env's car row act: the reference run with ONE column taken from the shared car
    instead (what a kernel that read the wrong constant would compute) differs from the true run, in the single steps and
    inside the call.  Under the controller the speed command is constant, so max_deceleration never acts there."""
    from tinycarlo_amd.randomization import CAR_COLUMNS
    true = fr.reference_run(kcode, True, "classes", feat)

    def differs(a, b):
        return any(not np.array_equal(a["state"][k], b["state"][k]) for k in fr.STATE_F) or \
            not np.array_equal(a["info"]["reward"], b["info"]["reward"])
    for j, name in enumerate(CAR_COLUMNS):
        if name == "max_deceleration" and feat & fr.FEAT_CTRL:
            continue
        other = fr.reference_run(kcode, True, "classes", feat, (j,))
        d = [differs(a, b) for a, b in zip(true["steps"], other["steps"])]
        assert any(d[:fr.N_SINGLE]) and any(d[fr.N_SINGLE:]), (kcode, feat, name, d)


@pytest.mark.parametrize("kcode,thick,fmt", [(5, True, "classes"), (9, False, "rgb"), (13, True, "classes")])
def test_every_layer_off_is_the_plain_batched_oracle(kcode, thick, fmt):
    from tinycarlo_amd import terms as T
    ref = fr.make_reference(kcode, thick, fmt, 0)
    o0 = ref.oracles[0]
    nodes, queue = fr.host_spawns(kcode)
    o = orc.Oracle(o0.map, ref.p, _camera_of(kcode, thick, fmt), orc.FMT_RGB if fmt == "rgb" else orc.FMT_CLASSES, fr.N_ENVS, threads=2)
    o.terms = [T.cte_termination(fr.MAX_CTE, 1)]
    o.spawn_queue = queue.copy()
    cc, man, _ = fr.case_inputs(kcode)

    def same(exp, label):
        for k in orc.STATE_DTYPE.names:
            assert np.array_equal(_bits(exp["state"][k]), _bits(o.state[k])), (label, "state", k)
        for k in orc.INFO_DTYPE.names:
            assert np.array_equal(_bits(exp["info"][k]), _bits(o.info[k])), (label, "info", k)
        assert np.array_equal(exp["obs"], o.obs), (label, "obs")
        assert np.array_equal(exp["needs_reset"], o.needs_reset) and np.array_equal(exp["spawn_cursor"], o.spawn_cursor), label
        assert exp["ep"] is None and exp["car"] is None and exp["steer"] is None

    o.reset(nodes)
    same(ref.reset(), "reset")
    respawns = 0
    for t in range(len(cc)):
        respawns += int(o.needs_reset.sum())
        o.step(cc[t], man[t], flags=orc.F_AUTORESET)
        same(ref.step(cc[t], man[t]), f"step {t}")
    assert respawns > fr.N_ENVS and o.obs.any()


def _camera_of(kcode, thick, fmt):
    import copy
    from tinycarlo_amd.camera import Camera
    return Camera(copy.deepcopy(fr.case_cfg(kcode, thick, fmt)["camera"]))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def test_episode_layer_equals_ref_on_simple_layout():
    """the inputs of test_gpu_episodes.closed_loop (simple_layout 64x64 classes, 64 envs, host spawns, staggered per-env
    limits) with the one fused term of the composed reference: `Ref` on an OracleVecEnv against FeatureRef's episode layer"""
    import test_gpu_episodes as te
    from oracle_backend import OracleVecEnv
    from tinycarlo_amd import terms as T
    Nn, steps, seed, max_cte = 64, 40, 5, 0.012
    per_env = 6 + (np.arange(Nn) % 5) * 4
    per_env[5] = 0
    length0 = (np.arange(Nn) * 3) % int(per_env.max())
    oenv = OracleVecEnv(te.cfg_for(), num_envs=Nn, autoreset=True, spawn="host")
    oenv.set_terms([T.cte_termination(max_cte, 1)])
    ref = fr.Ref(oenv, per_env)
    ref.reset(seed)
    ref.ep["length"][:] = length0
    comp = fr.FeatureRef(oenv.map, oenv.car_params, oenv.camera, orc.FMT_CLASSES, oenv._keep[0].numpy(),
                         oenv._aux["spawn_queue"].numpy(), max_cte, limit=per_env, length0=length0)
    comp.reset()
    cc, man = te.actions(steps, Nn, 2)
    for t in range(steps):
        a, b = ref.step(cc[t], man[t]), comp.step(cc[t], man[t])
        for k in fr.STATE_F + ("lp_len", "last_maneuver"):
            assert np.array_equal(_bits(a["state"][k]), _bits(b["state"][k])), (t, k)
        for k in ("cte", "heading_error", "reward", "status"):
            assert np.array_equal(_bits(a[k]), _bits(b["info"][k])), (t, k)
        for k in ("terminated", "truncated"):
            assert np.array_equal(a[k] != 0, b["info"][k] != 0), (t, k)
        assert np.array_equal(a["obs"].reshape(Nn, -1), b["obs"]), t
        assert np.array_equal(a["needs_reset"], b["needs_reset"]) and np.array_equal(a["spawn_cursor"], b["spawn_cursor"]), t
        for k in fr.EP_KEYS:
            assert np.array_equal(_bits(a["ep"][k]), _bits(b["ep"][k])), (t, "episode", k)
    ref.assert_not_vacuous()
    for k in ("respawns", "by_limit", "by_other"):
        assert np.array_equal(getattr(ref, k), getattr(comp.rules, k)), k
