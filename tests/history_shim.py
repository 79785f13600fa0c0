"""The frame-history rules of tinycarlo_amd/csrc/tc_collect.h (tc_collect_chain_step, tc_history_walk) built alone by the host
compiler, on top of tests/collect_shim.py's source: a shared library for ctypes (build_shim) that runs the link pass and the
resolve walk sequentially through whole calls, and, from the same source, a stand-alone program with its own main() for
sanitizer builds (build_program).  Test infrastructure."""
import ctypes as C
import os
import subprocess

import numpy as np

import collect_shim
from tinycarlo_amd import collect as col

SRC = collect_shim.SRC + r"""
// The link pass of one call, in front of shim_collect: looks at pending / age / counters without moving them.
extern "C" void shim_link(const tc_collect_desc* d, int32_t rows, const uint8_t* term, const uint8_t* trunc, int64_t* chain,
                          int64_t* link_rows) {
  const int N = d->num_envs;
  std::vector<uint8_t> pending(d->pending, d->pending + N);
  std::vector<int32_t> age(d->age, d->age + N);
  int64_t o = d->counters[TC_COLLECT_NEXT];
  for (int k = 0; k < rows; k++)
    for (int n = 0; n < N; n++) {
      const size_t at = (size_t)k * N + n;
      const int done = (term ? term[at] : 0) | (trunc ? trunc[at] : 0);
      const int respawn = pending[n] != 0;
      const int cand = tc_collect_env_step(&pending[n], &age[n], d->stride, done);
      link_rows[at] = tc_collect_chain_step(&chain[n], respawn, cand, cand ? o : -1);
      o += cand;
    }
}

extern "C" void shim_history(const int64_t* prev, const int64_t* ordinal, int64_t cap, int32_t mode, uint64_t seed,
                             const int64_t* index, int64_t B, int32_t T, int32_t pad, int64_t* slots, int32_t* valid) {
  for (int64_t b = 0; b < B; b++) valid[b] = tc_history_walk(prev, ordinal, mode, seed, cap, index[b], T, pad == TC_PAD_EDGE, slots + b * T);
}

#ifdef HISTORY_MAIN
// stand-alone form: every argument is a file of int64 head {mode, capacity, N, stride, seed, n_calls, n_T, B}, K[n_calls],
// T[n_T], then pending [N] (u8) of begin(), per call terminated and truncated [K][N] (u8), then what the definition expects
// afterwards: prev [capacity], chain [N], ordinal [capacity] (i64); then index [B] (i64) and per T, per pad (zero, edge)
// slots [B][T] (i64) and valid [B] (i32).  Frames are 4 zero bytes (collect_shim's program covers them).  Exit status 1
// on any difference, 2 on a malformed file.
static int run_history_file(const char* path) {
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
    if (n) memcpy(dst, buf.data() + cur, n);
    cur += n;
  };
  int64_t head[8] = {0};
  take(head, sizeof head);
  if (short_file || head[1] < 1 || head[2] < 1 || head[3] < 1 || head[5] < 1 || head[5] > 64 || head[6] < 1 || head[6] > 64 ||
      head[7] < 0 || head[1] > (1 << 24) || head[2] > (1 << 20) || head[7] > (1 << 24))
    return 2;
  const int mode = (int)head[0], N = (int)head[2], stride = (int)head[3], n_calls = (int)head[5], n_T = (int)head[6];
  const size_t cap = (size_t)head[1], B = (size_t)head[7], F = 4;
  std::vector<int64_t> Ks(n_calls), Ts(n_T);
  take(Ks.data(), n_calls * sizeof(int64_t));
  take(Ts.data(), n_T * sizeof(int64_t));
  std::vector<uint8_t> obs(cap * F, 0), pending(N), last((size_t)N * F, 0);
  std::vector<int64_t> ordinal(cap, -1), counters(4, 0), prev(cap, -1), chain(N, -1);
  std::vector<int32_t> env(cap, -1), age(N, 0);
  take(pending.data(), N);
  tc_collect_desc d;
  memset(&d, 0, sizeof d);
  d.capacity = (int64_t)cap; d.num_envs = N; d.stride = stride; d.mode = mode; d.n_columns = 1; d.seed = (uint64_t)head[4];
  d.frame_bytes = (int64_t)F; d.obs = obs.data(); d.ordinal = ordinal.data(); d.env = env.data();
  d.pending = pending.data(); d.age = age.data(); d.last = last.data(); d.counters = counters.data();
  d.columns[0].dst = prev.data(); d.columns[0].elem_size = 8;
  for (int c = 0; c < n_calls && !short_file; c++) {
    const size_t K = (size_t)Ks[c], KN = K * N;
    if (K < 1 || K > 4096) return 2;
    std::vector<uint8_t> rows(KN * F, 0), te(KN), tr(KN);
    std::vector<int64_t> link(KN);
    take(te.data(), KN); take(tr.data(), KN);
    if (short_file) break;
    d.columns[0].src = link.data();
    shim_link(&d, (int32_t)K, te.data(), tr.data(), chain.data(), link.data());
    shim_collect(&d, (int32_t)K, rows.data(), te.data(), tr.data());
  }
  int wrong = 0;
  auto same = [&](const void* have, size_t n, const char* what) {
    if (cur + n > buf.size()) { short_file = true; return; }
    if (n && memcmp(have, buf.data() + cur, n) != 0) { wrong++; printf("differs: %s\n", what); }
    cur += n;
  };
  same(prev.data(), cap * 8, "prev"); same(chain.data(), (size_t)N * 8, "chain"); same(ordinal.data(), cap * 8, "ordinal");
  std::vector<int64_t> index(B);
  take(index.data(), B * 8);
  long long full = 0;
  for (int i = 0; i < n_T && !short_file; i++) {
    const int64_t T = Ts[i];
    if (T < 1 || T > 4096) return 2;
    for (int pad = 0; pad < 2; pad++) {
      std::vector<int64_t> slots(B * (size_t)T);
      std::vector<int32_t> valid(B);
      shim_history(prev.data(), ordinal.data(), (int64_t)cap, mode, (uint64_t)head[4], index.data(), (int64_t)B, (int32_t)T, pad,
                   slots.data(), valid.data());
      same(slots.data(), slots.size() * 8, "slots"); same(valid.data(), B * 4, "valid");
      for (size_t b = 0; b < B; b++) full += valid[b] == T;
    }
  }
  if (short_file || cur != buf.size()) return 2;
  printf("calls %d, next %lld, samples %lld, full %lld, wrong %d\n", n_calls, (long long)counters[1], (long long)B, full, wrong);
  return wrong ? 1 : 0;
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  for (int i = 1; i < argc; i++) {
    const int rc = run_history_file(argv[i]);
    if (rc) return rc;
  }
  return 0;
}
#endif
"""


def _write_src(d):
    src = os.path.join(str(d), "history_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d):
    """-> ctypes library of the shim built in directory d (collect_shim's functions included)"""
    src = _write_src(d)
    lib = os.path.join(str(d), "libtc_history_shim.so")
    subprocess.check_call(["c++"] + collect_shim.FLAGS + ["-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    L.shim_collect.restype = None
    L.shim_collect.argtypes = [C.POINTER(col.CollectDescC), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.shim_link.restype = None
    L.shim_link.argtypes = [C.POINTER(col.CollectDescC), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.shim_history.restype = None
    L.shim_history.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_uint64, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                               C.c_void_p, C.c_void_p]
    return L


def build_program(d, sanitize=True):
    """-> path of the stand-alone program (its own main), with -fsanitize=address,undefined unless told otherwise"""
    src = _write_src(d)
    exe = os.path.join(str(d), "history_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["c++"] + collect_shim.FLAGS + san + ["-DHISTORY_MAIN", "-o", exe, src])
    return exe


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_call(L, state, rows, stride, overflow, seed):
    """shim_link + shim_collect on a reference state with links (reference_state(history=True)), in place: the links go
    through shim_collect as one more 8-byte column, as they do on the device"""
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
    link = np.full((K, N), -7, dtype=np.int64)
    j = len(keep)
    d.columns[j].src, d.columns[j].dst, d.columns[j].elem_size = _ptr(link), _ptr(state["prev"]), 8
    d.n_columns = j + 1
    d.pending, d.age, d.last, d.counters = _ptr(state["pending"]), _ptr(state["age"]), _ptr(state["last"]), _ptr(counters)
    te = np.ascontiguousarray(rows["terminated"], dtype=np.uint8) if rows.get("terminated") is not None else None
    tr = np.ascontiguousarray(rows["truncated"], dtype=np.uint8) if rows.get("truncated") is not None else None
    pte, ptr_ = (_ptr(te) if te is not None else None), (_ptr(tr) if tr is not None else None)
    L.shim_link(C.byref(d), K, pte, ptr_, _ptr(state["chain"]), _ptr(link))
    L.shim_collect(C.byref(d), K, _ptr(obs), pte, ptr_)
    state["count"], state["next_ordinal"], state["dropped"] = int(counters[0]), int(counters[1]), int(counters[2])
    return link


def run_history(L, state, index, T, pad, overflow, seed):
    """shim_history on a reference state -> (slots [B, T], valid [B])"""
    index = np.ascontiguousarray(index, dtype=np.int64)
    B = len(index)
    slots, valid = np.full((B, T), -9, dtype=np.int64), np.full(B, -9, dtype=np.int32)
    L.shim_history(_ptr(state["prev"]), _ptr(state["ordinal"]), len(state["ordinal"]), col.OVERFLOW[overflow], seed, _ptr(index), B, T,
                   col.PAD[pad], _ptr(slots), _ptr(valid))
    return slots, valid


def program_input(case, st, index, Ts):
    """the stand-alone program's input file for a collect_cases.Case, the reference state `st` after its calls, the sample
    index and the history lengths, as bytes"""
    index = np.ascontiguousarray(index, dtype=np.int64)
    head = np.array([col.OVERFLOW[case.overflow], case.capacity, case.N, case.stride, case.seed, len(case.Ks), len(Ts), len(index)]
                    + list(case.Ks) + list(Ts), dtype=np.int64)
    parts = [head.tobytes(), case.begin_pending.astype(np.uint8).tobytes()]
    for rows in case.calls:
        parts += [np.ascontiguousarray(rows[k], dtype=np.uint8).tobytes() for k in ("terminated", "truncated")]
    parts += [st[k].tobytes() for k in ("prev", "chain", "ordinal")]
    parts.append(index.tobytes())
    for T in Ts:
        for pad in ("zero", "edge"):
            h = col.history_reference(st, index, T, pad, case.overflow, case.seed)
            parts += [h["slots"].tobytes(), h["valid"].tobytes()]
    return b"".join(parts)
