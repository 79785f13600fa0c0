"""Which steps of a call compute the lane-line distances ("phase B" of the simulate kernels): the plan's bit
CallPlan::info_every (tinycarlo_amd/csrc/tc_plan.h), run on the CPU through a host shim like tests/test_plan_cpu.py's.

The rule, restated here from who reads a step's distances: the rollout's laneline_distances / nearest_edge rows, a
term of one of the three lane-line kinds, or the switch TC_INFO_EVERY_STEP.  With none of them only the last step of
every launch computes them (the env's buffers hold that step's).  The bit belongs to the CALL: every launch a long call is
cut into (streamed segments, chunks) is given the same one.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from common import ROOT
from tinycarlo_amd import terms as T

SHIM = r"""
#include "tc_plan.h"
// in: n rows of 10 ints: dist rows, ne rows, n_terms, kind of term 0, kind of term 1, the switch, nsteps, TC_STREAM,
// TC_MULTI_SPLIT, TC_ENV_GROUPED; out: n rows of 3: CallPlan::info_every, CallPlan::steps, CallPlan::streamed
extern "C" void info_need(const int* in, int n, int* out) {
  for (int i = 0; i < n; i++, in += 10, out += 3) {
    CallInputs c;
    c.fuse = 1, c.multi_split = in[8], c.env_grouped = in[9], c.pipe = 1, c.stream = in[7], c.chunk = 16;
    c.kvar = 5, c.packed = false, c.ring_rows = 16, c.streamed_rows = 128, c.st_words = true;
    c.flags = 0, c.no_frame_flags = 0x401, c.nsteps = in[6], c.obs = true, c.all = true;
    c.info_rows = in[0] != 0 || in[1] != 0;
    bool reads = false;  // (as tc_env_set_terms keeps it on the handle)
    for (int t = 0; t < in[2]; t++) reads = reads || term_reads_distances(in[3 + t]);
    c.info_terms = reads;
    c.info_every = in[5];
    const CallPlan p = plan_call(c);
    out[0] = p.info_every, out[1] = p.steps, out[2] = p.streamed;
  }
}
extern "C" int reads_distances(int kind) { return term_reads_distances(kind) ? 1 : 0; }
// a CallInputs that says nothing about the distances' readers: the last step only
extern "C" int default_bit() {
  CallInputs c;
  c.fuse = 1, c.multi_split = 1, c.env_grouped = 1, c.pipe = 1, c.stream = 1, c.chunk = 16, c.kvar = 5, c.packed = false;
  c.ring_rows = 16, c.streamed_rows = 128, c.st_words = true, c.flags = 0, c.no_frame_flags = 0x401, c.nsteps = 128;
  c.obs = true, c.all = true;
  return plan_call(c).info_every ? 1 : 0;
}
"""

KINDS = (T.LANELINE_SPARSE_REWARD, T.LANELINE_LINEAR_REWARD, T.CTE_SPARSE_REWARD, T.CTE_LINEAR_REWARD,
         T.LANELINE_CROSSING_TERMINATION, T.CTE_TERMINATION, T.CRASH_TERMINATION)
LANELINE_KINDS = {T.LANELINE_SPARSE_REWARD, T.LANELINE_LINEAR_REWARD, T.LANELINE_CROSSING_TERMINATION}
ROWS = {"dist": (1, 0), "ne": (0, 1), "neither": (0, 0)}
# (n_terms, kind 0, kind 1): no term, each of the 7 kinds alone, a CTE term plus a lane-line term (either order)
STACKS = [(0, 0, 0)] + [(1, k, 0) for k in KINDS] + [(2, T.CTE_LINEAR_REWARD, T.LANELINE_CROSSING_TERMINATION),
                                                     (2, T.LANELINE_SPARSE_REWARD, T.CTE_TERMINATION)]
# (TC_STREAM, TC_MULTI_SPLIT, TC_ENV_GROUPED): streamed, chunked, one wavefront per env, fused
FORMS = [(1, 1, 1), (0, 1, 1), (1, 1, 0), (1, 0, 1)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("tc_info_need")
    src, lib = os.path.join(str(d), "shim.cpp"), os.path.join(str(d), "libtc_info_need.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc"), "-o", lib, src])
    return C.CDLL(lib)


def test_kinds_that_read_distances(shim):
    assert len(KINDS) == 7 and KINDS == tuple(range(1, 8))
    for k in KINDS:
        assert bool(shim.reads_distances(k)) == (k in LANELINE_KINDS), k
    for k in (0, 8, -1):
        assert not shim.reads_distances(k), k


def test_inputs_default_to_last_step_only(shim):
    assert shim.default_bit() == 0


@pytest.mark.parametrize("nsteps", [1, 20, 128, 300])
def test_info_bit_over_every_combination(shim, nsteps):
    combos = list(itertools.product(ROWS, STACKS, (0, 1), FORMS))
    assert len(combos) == 3 * 10 * 2 * len(FORMS)
    rows = np.array([[*ROWS[r], *st, sw, nsteps, *form] for r, st, sw, form in combos], dtype=np.int32)
    out = np.zeros((len(rows), 3), dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    shim.info_need(rows.ctypes.data_as(ip), len(rows), out.ctypes.data_as(ip))
    seen = set()
    for (r, st, sw, form), (bit, steps, streamed) in zip(combos, out.tolist()):
        reads = any(k in LANELINE_KINDS for k in st[1:1 + st[0]])
        want = r != "neither" or reads or sw == 1
        assert bool(bit) == want, (r, st, sw, form, nsteps)
        # the launches of the call: steps [c0, c0 + min(steps, rest)) each.  The plan has ONE bit for all of them (the
        # launchers copy it into every launch's flags, step_args_at), so it cannot differ between the launches of a call;
        # what is checked here is that the answer does not depend on how the call is cut (the form, the call's length).
        assert 1 <= steps <= nsteps
        launches = [(c0, min(steps, nsteps - c0)) for c0 in range(0, nsteps, steps)]
        assert sum(n for _, n in launches) == nsteps
        seen.add((len(launches) > 1, bool(streamed)))
    if nsteps == 300:  # three streamed segments (128 + 128 + 44) and 19 chunks: both kinds of split occur
        assert (True, True) in seen and (True, False) in seen
        streamed_steps = {s for (r, st, sw, form), (b, s, sd) in zip(combos, out.tolist()) if sd}
        assert streamed_steps == {128}
