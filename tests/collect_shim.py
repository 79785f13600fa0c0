"""tinycarlo_amd/csrc/tc_collect.h (and tc_rng.h's tc_replace_slot) built alone by the host compiler: a shared library for
ctypes (build_shim) that runs whole calls sequentially through the header's rules, and, from the same source, a stand-alone
program with its own main() for sanitizer builds (build_program).  Test infrastructure."""
import ctypes as C
import os
import subprocess

import numpy as np

from tinycarlo_amd import collect as col

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include "tc_collect.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" uint32_t shim_replace_slot(uint64_t seed, uint64_t o, uint32_t cap) { return tc_replace_slot(seed, o, cap); }
extern "C" int64_t shim_scratch_size(int32_t rows, int32_t n) { return tc_collect_scratch_size(rows, n); }

// One call, in the kernels' order of passes: flags (rules 1-3), [random: claims], copies, carry, counters.
extern "C" void shim_collect(const tc_collect_desc* d, int32_t rows, const uint8_t* obs_rows, const uint8_t* term, const uint8_t* trunc) {
  const int N = d->num_envs;
  const size_t F = (size_t)d->frame_bytes;
  std::vector<uint8_t> flag((size_t)rows * N);
  int64_t c = 0;
  for (int k = 0; k < rows; k++)
    for (int n = 0; n < N; n++) {
      const size_t at = (size_t)k * N + n;
      const int done = (term ? term[at] : 0) | (trunc ? trunc[at] : 0);
      flag[at] = (uint8_t)tc_collect_env_step(&d->pending[n], &d->age[n], d->stride, done);
      c += flag[at];
    }
  const int64_t o0 = d->counters[TC_COLLECT_NEXT];
  if (d->mode == TC_COLLECT_RANDOM) {
    int64_t o = o0;
    for (size_t at = 0; at < flag.size(); at++)
      if (flag[at]) {
        const int64_t slot = tc_collect_slot(d->mode, d->seed, o, d->capacity);
        if (slot >= 0 && d->ordinal[slot] < o) d->ordinal[slot] = o;
        o++;
      }
  }
  int64_t o = o0;
  for (int k = 0; k < rows; k++)
    for (int n = 0; n < N; n++) {
      const size_t at = (size_t)k * N + n;
      if (!flag[at]) continue;
      const int64_t slot = tc_collect_slot(d->mode, d->seed, o, d->capacity);
      const int64_t claimed = d->mode == TC_COLLECT_RANDOM && slot >= 0 ? d->ordinal[slot] : o;
      if (slot >= 0 && tc_collect_writes(d->mode, o, o0, c, d->capacity, claimed)) {
        memcpy(d->obs + (size_t)slot * F, k == 0 ? d->last + (size_t)n * F : obs_rows + (at - N) * F, F);
        if (d->next_obs) memcpy(d->next_obs + (size_t)slot * F, obs_rows + at * F, F);
        for (int j = 0; j < d->n_columns; j++) {
          const size_t e = (size_t)d->columns[j].elem_size;
          memcpy((char*)d->columns[j].dst + (size_t)slot * e, (const char*)d->columns[j].src + at * e, e);
        }
        d->env[slot] = n;
        d->ordinal[slot] = o;
      }
      o++;
    }
  memcpy(d->last, obs_rows + (size_t)(rows - 1) * N * F, (size_t)N * F);
  tc_collect_advance(d->mode, c, d->capacity, d->counters);
}

#ifdef COLLECT_MAIN
// stand-alone form: every argument is a file of int64 head {mode, capacity, N, stride, F, next_obs, seed, n_calls, K[n_calls]}, then
// the begin state (pending [N], last [N][F]), then per call obs [K][N][F], terminated, truncated [K][N], and the columns flag
// (u8), maneuver (i32), steer (f64) [K][N], then what the definition expects afterwards: obs, [next_obs], ordinal, env, flag,
// maneuver, steer, pending, age, last, counters[3].  Destinations start as 0xFF bytes.  Exit status 1 on any difference.
static int run_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return 2;
  std::vector<uint8_t> buf;
  uint8_t tmp[65536];
  size_t got;
  while ((got = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  fclose(f);
  size_t cur = 0;
  bool short_file = false;
  auto take = [&](void* dst, size_t n) {
    if (cur + n > buf.size()) { short_file = true; return; }
    memcpy(dst, buf.data() + cur, n);
    cur += n;
  };
  int64_t head[8] = {0};
  take(head, sizeof head);
  if (short_file || head[2] < 1 || head[1] < 1 || head[4] < 4 || head[7] < 1 || head[7] > 64) return 2;
  const int mode = (int)head[0], N = (int)head[2], stride = (int)head[3], n_calls = (int)head[7];
  const size_t cap = (size_t)head[1], F = (size_t)head[4];
  const bool nx = head[5] != 0;
  std::vector<int64_t> Ks(n_calls);
  take(Ks.data(), n_calls * sizeof(int64_t));
  std::vector<uint8_t> obs(cap * F, 0xFF), next(nx ? cap * F : 0, 0xFF), cflag(cap, 0xFF), pending(N), last((size_t)N * F);
  std::vector<int64_t> ordinal(cap, -1), counters(4, 0);
  std::vector<int32_t> env(cap, -1), cman(cap, -1), age(N, 0);
  std::vector<double> csteer(cap);
  memset(csteer.data(), 0xFF, cap * sizeof(double));
  take(pending.data(), N);
  take(last.data(), (size_t)N * F);
  tc_collect_desc d;
  memset(&d, 0, sizeof d);
  d.capacity = (int64_t)cap; d.num_envs = N; d.stride = stride; d.mode = mode; d.n_columns = 3; d.seed = (uint64_t)head[6];
  d.frame_bytes = (int64_t)F; d.obs = obs.data(); d.next_obs = nx ? next.data() : NULL; d.ordinal = ordinal.data(); d.env = env.data();
  d.pending = pending.data(); d.age = age.data(); d.last = last.data(); d.counters = counters.data();
  d.columns[0].dst = cflag.data(); d.columns[0].elem_size = 1;
  d.columns[1].dst = cman.data(); d.columns[1].elem_size = 4;
  d.columns[2].dst = csteer.data(); d.columns[2].elem_size = 8;
  for (int c = 0; c < n_calls && !short_file; c++) {
    const size_t K = (size_t)Ks[c], KN = K * N;
    if (K < 1 || K > 4096) return 2;
    std::vector<uint8_t> rows(KN * F), te(KN), tr(KN), fl(KN);
    std::vector<int32_t> man(KN);
    std::vector<double> st(KN);
    take(rows.data(), KN * F); take(te.data(), KN); take(tr.data(), KN);
    take(fl.data(), KN); take(man.data(), KN * 4); take(st.data(), KN * 8);
    if (short_file) break;
    d.columns[0].src = fl.data(); d.columns[1].src = man.data(); d.columns[2].src = st.data();
    shim_collect(&d, (int32_t)K, rows.data(), te.data(), tr.data());
  }
  int wrong = 0;
  auto same = [&](const void* have, size_t n, const char* what) {
    if (cur + n > buf.size()) { short_file = true; return; }
    if (memcmp(have, buf.data() + cur, n) != 0) { wrong++; printf("differs: %s\n", what); }
    cur += n;
  };
  same(obs.data(), cap * F, "obs");
  if (nx) same(next.data(), cap * F, "next_obs");
  same(ordinal.data(), cap * 8, "ordinal"); same(env.data(), cap * 4, "env");
  same(cflag.data(), cap, "flag"); same(cman.data(), cap * 4, "maneuver"); same(csteer.data(), cap * 8, "steer");
  same(pending.data(), N, "pending"); same(age.data(), (size_t)N * 4, "age"); same(last.data(), (size_t)N * F, "last");
  same(counters.data(), 24, "counters");
  if (short_file || cur != buf.size()) return 2;
  printf("calls %d, kept %lld, next %lld, dropped %lld, wrong %d\n", n_calls, (long long)counters[0], (long long)counters[1],
         (long long)counters[2], wrong);
  return wrong ? 1 : 0;
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int i = 1; i < argc; i++) {
    const int rc = run_file(argv[i]);
    if (rc) return rc;
  }
  return 0;
}
#endif
"""

FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "tinycarlo_amd", "csrc")]


def _write_src(d):
    src = os.path.join(str(d), "collect_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d):
    """-> ctypes library of the shim built in directory d"""
    src = _write_src(d)
    lib = os.path.join(str(d), "libtc_collect_shim.so")
    subprocess.check_call(["c++"] + FLAGS + ["-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.shim_replace_slot.restype = C.c_uint32
    L.shim_replace_slot.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    L.shim_scratch_size.restype = C.c_int64
    L.shim_scratch_size.argtypes = [C.c_int32, C.c_int32]
    L.shim_collect.restype = None
    L.shim_collect.argtypes = [C.POINTER(col.CollectDescC), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def build_program(d, sanitize=True):
    """-> path of the stand-alone program (its own main), with -fsanitize=address,undefined unless told otherwise"""
    src = _write_src(d)
    exe = os.path.join(str(d), "collect_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["c++"] + FLAGS + san + ["-DCOLLECT_MAIN", "-o", exe, src])
    return exe


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_call(L, state, rows, stride, overflow, seed):
    """shim_collect on a reference state (numpy arrays of tinycarlo_amd.collect.reference_state), in place"""
    d = col.CollectDescC()
    counters = np.array([state["count"], state["next_ordinal"], state["dropped"], 0], dtype=np.int64)
    obs = np.ascontiguousarray(rows["obs"])
    K, N = obs.shape[:2]
    d.capacity, d.num_envs, d.stride, d.mode = len(state["ordinal"]), N, stride, col.OVERFLOW[overflow]
    d.seed, d.frame_bytes = seed, int(np.prod(obs.shape[2:]))
    d.obs, d.next_obs = _ptr(state["obs"]), (_ptr(state["next_obs"]) if state["next_obs"] is not None else None)
    d.ordinal, d.env = _ptr(state["ordinal"]), _ptr(state["env"])
    keep = []
    for j, (name, dst) in enumerate(state["cols"].items()):
        src = np.ascontiguousarray(rows[name], dtype=dst.dtype)
        keep.append(src)
        d.columns[j].src, d.columns[j].dst, d.columns[j].elem_size = _ptr(src), _ptr(dst), dst.dtype.itemsize
    d.n_columns = len(keep)
    d.pending, d.age, d.last, d.counters = _ptr(state["pending"]), _ptr(state["age"]), _ptr(state["last"]), _ptr(counters)
    te = np.ascontiguousarray(rows["terminated"], dtype=np.uint8) if rows.get("terminated") is not None else None
    tr = np.ascontiguousarray(rows["truncated"], dtype=np.uint8) if rows.get("truncated") is not None else None
    L.shim_collect(C.byref(d), K, _ptr(obs), _ptr(te) if te is not None else None, _ptr(tr) if tr is not None else None)
    state["count"], state["next_ordinal"], state["dropped"] = int(counters[0]), int(counters[1]), int(counters[2])
    return int(counters[3])


def program_input(case):
    """the stand-alone program's input file for a collect_cases.Case (columns flag / maneuver / steer), as bytes"""
    head = np.array([col.OVERFLOW[case.overflow], case.capacity, case.N, case.stride, case.F, int(case.next_obs), case.seed,
                     len(case.Ks)] + list(case.Ks), dtype=np.int64)
    parts = [head.tobytes(), case.begin_pending.astype(np.uint8).tobytes(), case.begin_obs.tobytes()]
    for rows in case.calls:
        parts += [np.ascontiguousarray(rows[k]).tobytes() for k in ("obs", "terminated", "truncated", "flag", "maneuver", "steer")]
    st = case.reference()
    parts.append(st["obs"].tobytes())
    if case.next_obs:
        parts.append(st["next_obs"].tobytes())
    parts += [st[k].tobytes() for k in ("ordinal", "env")] + [st["cols"][k].tobytes() for k in ("flag", "maneuver", "steer")]
    parts += [st[k].tobytes() for k in ("pending", "age", "last")]
    parts.append(np.array([st["count"], st["next_ordinal"], st["dropped"]], dtype=np.int64).tobytes())
    return b"".join(parts)
