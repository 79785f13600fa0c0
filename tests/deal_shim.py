"""The raster stage's item dealing (tinycarlo_amd/csrc/tc_deal.h) built by the host compiler: the scan form, its 64 lanes
emulated, beside the literal binary search -- as a shared library for ctypes (build_shim) and as a stand-alone program with
its own main() for sanitizer builds (build_program).  Test infrastructure of tests/test_deal_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tinycarlo_amd", "csrc")
FLAGS = ["-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC]

SRC = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tc_deal.h"

// Deal a table of n_tab entries (cnt[0 .. n), zeros behind them, as the kernel's tables are padded) pass by pass, as the
// kernel does: owner[c], offset[c] for every item c < total.  Returns the number of passes.
extern "C" int deal_scan(const int* cnt, int n, int n_tab, int* owner, int* offset) {
  std::vector<int> pre(n_tab), num(n_tab, 0);
  int total = 0;
  for (int t = 0; t < n_tab; t++) {
    if (t < n) num[t] = cnt[t];
    pre[t] = total;
    total += num[t];
  }
  int scratch[TC_DEAL_LANES], words[TC_DEAL_LANES], carry = 0, passes = 0;
  for (int c0 = 0; c0 < total; c0 += TC_DEAL_LANES, passes++) {
    carry = tc_deal_pass(pre.data(), num.data(), n_tab, c0, carry, scratch, words);
    for (int l = 0; l < TC_DEAL_LANES && c0 + l < total; l++) {
      owner[c0 + l] = tc_deal_owner(words[l]);
      offset[c0 + l] = tc_deal_offset(words[l], c0 + l);
    }
  }
  return passes;
}
// the specification: the binary search through the table of prefixes
extern "C" void deal_search(const int* cnt, int n, int n_tab, int* owner, int* offset) {
  std::vector<int> pre(n_tab);
  int total = 0;
  for (int t = 0; t < n_tab; t++) {
    pre[t] = total;
    total += t < n ? cnt[t] : 0;
  }
  for (int c = 0; c < total; c++) {
    owner[c] = tc_deal_search(pre.data(), n_tab, c);
    offset[c] = c - pre[owner[c]];
  }
}
// items on which the two forms differ (0 = equal), plus items whose owner has no such item (never, if both are right)
extern "C" long deal_mismatches(const int* cnt, int n, int n_tab) {
  int total = 0;
  for (int t = 0; t < n; t++) total += cnt[t];
  std::vector<int> o1(total + 1), f1(total + 1), o2(total + 1), f2(total + 1);
  deal_scan(cnt, n, n_tab, o1.data(), f1.data());
  deal_search(cnt, n, n_tab, o2.data(), f2.data());
  long bad = 0;
  for (int c = 0; c < total; c++) {
    bad += o1[c] != o2[c] || f1[c] != f2[c];
    bad += o1[c] < 0 || o1[c] >= n || f1[c] < 0 || f1[c] >= cnt[o1[c]];
  }
  return bad;
}
// every count vector of 1 .. max_n entries with counts 0 .. max_cnt, none left out, each as a table of exactly its entries
// and padded to 64 and 128: vectors[0] = how many; returns the mismatches
extern "C" long deal_exhaustive(int max_n, int max_cnt, long* vectors) {
  long bad = 0, nv = 0;
  std::vector<int> cnt(max_n, 0);
  for (int n = 1; n <= max_n; n++) {
    for (int i = 0; i < n; i++) cnt[i] = 0;
    for (;;) {
      bad += deal_mismatches(cnt.data(), n, n) + deal_mismatches(cnt.data(), n, 64) + deal_mismatches(cnt.data(), n, 128);
      nv++;
      int i = 0;
      while (i < n && cnt[i] == max_cnt) cnt[i++] = 0;
      if (i == n) break;
      cnt[i]++;
    }
  }
  *vectors = nv;
  return bad;
}

#ifdef DEAL_MAIN
// stand-alone form: the exhaustive vectors, random tables of 64 and 128 entries with totals up to 1000 (several passes,
// windows no entry starts in), and all items in one entry.  Exit status 1 on any mismatch; prints the counts.
static unsigned long long lcg_state = 0x9e3779b97f4a7c15ull;
static unsigned lcg() {
  lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)(lcg_state >> 33);
}
int main() {
  long nv = 0, bad = deal_exhaustive(6, 5, &nv);
  long nr = 0;
  for (int rep = 0; rep < 4000; rep++) {
    const int n = (rep & 1) ? 128 : 64;
    std::vector<int> cnt(n, 0);
    const int total = 1 + (int)(lcg() % 1000), live = 1 + (int)(lcg() % n);  // items spread over `live` random entries
    for (int i = 0; i < total; i++) cnt[(lcg() % live) * (n / live) % n]++;
    bad += deal_mismatches(cnt.data(), n, n);
    nr++;
  }
  for (int n = 64; n <= 128; n += 64)
    for (int at = 0; at < n; at++) {
      std::vector<int> cnt(n, 0);
      cnt[at] = 1 + (at * 37) % 1000;
      bad += deal_mismatches(cnt.data(), n, n);
      nr++;
    }
  printf("exhaustive %ld, random and single-entry %ld, mismatches %ld\n", nv, nr, bad);
  return bad ? 1 : 0;
}
#endif
"""


def _write_src(d):
    src = os.path.join(str(d), "deal_shim.cpp")
    with open(src, "w") as f:
        f.write(SRC)
    return src


def build_shim(d):
    """-> ctypes library with deal_scan, deal_search, deal_mismatches, deal_exhaustive"""
    src = _write_src(d)
    lib = os.path.join(str(d), "libtc_deal.so")
    subprocess.check_call(["c++"] + FLAGS + ["-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    ip = C.POINTER(C.c_int32)
    L.deal_scan.argtypes = [ip, C.c_int, C.c_int, ip, ip]
    L.deal_search.argtypes = [ip, C.c_int, C.c_int, ip, ip]
    L.deal_mismatches.restype = C.c_long
    L.deal_mismatches.argtypes = [ip, C.c_int, C.c_int]
    L.deal_exhaustive.restype = C.c_long
    L.deal_exhaustive.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_long)]
    return L


def build_program(d, sanitize=True):
    """-> path of the stand-alone program (its own main), with -fsanitize=address,undefined unless told otherwise"""
    src = _write_src(d)
    exe = os.path.join(str(d), "deal_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["c++"] + FLAGS + san + ["-DDEAL_MAIN", "-o", exe, src])
    return exe


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def deal(L, cnt, n_tab=None, form="scan"):
    """(owner, offset, passes) of every item of the table `cnt` (padded with zeros to n_tab entries) by the given form"""
    cnt = np.ascontiguousarray(cnt, dtype=np.int32)
    n_tab = len(cnt) if n_tab is None else n_tab
    total = int(cnt.sum())
    owner, offset = np.zeros(total + 1, np.int32), np.zeros(total + 1, np.int32)
    passes = None
    if form == "scan":
        passes = L.deal_scan(_ip(cnt), len(cnt), n_tab, _ip(owner), _ip(offset))
    else:
        L.deal_search(_ip(cnt), len(cnt), n_tab, _ip(owner), _ip(offset))
    return owner[:total], offset[:total], passes
