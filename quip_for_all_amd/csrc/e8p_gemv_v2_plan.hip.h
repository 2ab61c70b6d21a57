// Launch plans of the K-splitting GEMV (e8p_gemv_v2.hip: byte tables, e8p_gemv_v2n.hip: nibble mode).  A plan is pure
// host arithmetic on (ns, k, tune): each kernel keeps its own candidate search -- the byte kernel's (rep, ksplit) cost
// search, the nibble kernel's first fit -- and shares the row split, the wave / run-length rule and the argument fill
// below.  quip_e8p_gemv_v2_plan() (quip_internal.h) hands a plan out; tests/golden/gemv_v2_plans.json pins them, because
// integer sums make y bit identical under any plan and a planning change would otherwise only show as speed.
#pragma once
#include "quip_device.hip.h"
#include "quip_internal.h"

namespace quip {

constexpr int kV2MaxG = 3;   // problems per launch (kMaxG / kMaxGN of the two kernels)

struct GemvV2Plan {   // the order of quip_e8p_gemv_v2_plan's out[13]; fields a failed plan never reached stay 0
  int rc = QUIP_ERR_UNSUPPORTED;
  int rep = 0, slots = 0, ksplit = 0, nrb = 0, spw = 0, rpb[kV2MaxG] = {0, 0, 0};
  int runlen = 0, rpr_inv = 0, threads = 0, lds = 0;
};
GemvV2Plan e8p_gemv_v2n_plan(const int* ns, int count, int k, const GemvTune& tune, bool have_ws);

// rows per workgroup of every problem for about `nrb_c` row blocks, in multiples of `granule` (rows of an accumulator
// unit: 4 byte mode, 8 nibble mode); the accumulator rows must fit: more row blocks until they do
struct V2RowSplit {
  int rpb[kV2MaxG] = {0, 0, 0};
  int rows = 0, units = 0, nrb = 1;
};
inline V2RowSplit v2_row_split(const int* ns, int G, int nrb_c, int granule) {
  V2RowSplit s;
  if (nrb_c < 1) nrb_c = 1;
  for (;;) {
    s.rows = 0; s.units = 0; s.nrb = 1;
    for (int p = 0; p < G; ++p) {
      int v = (ns[p] + nrb_c - 1) / nrb_c;
      v = (v + granule - 1) & ~(granule - 1);
      s.rpb[p] = v;
      s.rows += v;
      s.units += v / granule;
      const int nb = (ns[p] + v - 1) / v;
      s.nrb = nb > s.nrb ? nb : s.nrb;
    }
    if (s.rows <= 1024) return s;
    nrb_c *= 2;
  }
}

// the chosen candidate into the plan; false: the K split needs a workspace and there is none (rc says so)
inline bool v2_plan_split(GemvV2Plan& pl, int rep, int segs, int spw, const V2RowSplit& s, bool have_ws) {
  pl.rep = rep; pl.spw = spw; pl.nrb = s.nrb;
  pl.ksplit = (segs + spw - 1) / spw;
  for (int p = 0; p < kV2MaxG; ++p) pl.rpb[p] = s.rpb[p];
  if (pl.ksplit > 1 && !have_ws) pl.rc = QUIP_ERR_NULL_POINTER;
  return pl.rc != QUIP_ERR_NULL_POINTER;
}

// waves, run length and its reciprocal word.  units: accumulator units of a workgroup; seg_k16: k16 indices of a segment
// (64 / 32); runs_per_wave: what the run length should leave every wave (3 / 2, measured per kernel)
inline void v2_plan_waves(GemvV2Plan& pl, int G, int units, const GemvTune& tune, int seg_k16, int runs_per_wave) {
  const int spw = pl.spw;
  // 16 waves for long streams; 12 when a workgroup has few units (8192^2: 64 units, 7.2 vs 7.9 us with 16)
  int waves = tune.max_waves > 0 ? tune.max_waves : (units * spw >= 128 ? 16 : 12);
  if (waves < 8) waves = 8;     // the table build uses waves 0..7
  if (waves > 16) waves = 16;
  while (waves < 16 && spw * seg_k16 > (G == 1 ? 2 : 1) * waves * 64) ++waves;   // k16 indices per thread
  // run length: the longest (fewest LDS flushes, longest contiguous reads) that still leaves about runs_per_wave runs per wave
  int runlen = tune.digits > 0 ? tune.digits : spw;
  if (tune.digits <= 0)
    while (runlen > pl.slots && units * ((spw + runlen - 1) / runlen) < runs_per_wave * waves) runlen = (runlen + 1) / 2;
  if (runlen > spw) runlen = spw;
  if (runlen < 1) runlen = 1;
  pl.runlen = runlen;
  const int rpr = (spw + runlen - 1) / runlen;
  pl.rpr_inv = (rpr << 24) | (((1 << 20) / rpr + 1) & 0xffffff);
  pl.threads = waves * 64;
}

// the fields V2Args and V2nArgs share
template <class Args>
void v2_fill_args(Args& a, const GemvV2Plan& pl, int G, const void* const* planes, const void* const* qidxs, const void* grid,
                  void* const* ys, void* ws, const int* ns, int k, int segs, void* dbg) {
  size_t ws_off = 0;
  for (int p = 0; p < kV2MaxG; ++p) {
    const int pp = p < G ? p : 0;
    a.W[p] = reinterpret_cast<const uint4*>(qidxs[pp]);
    a.planes[p] = reinterpret_cast<const uint8_t*>(planes[pp]);
    a.y[p] = reinterpret_cast<f16*>(ys[pp]);
    a.N[p] = ns[pp];
    a.rpb[p] = pl.rpb[pp];
    a.ws[p] = ws ? reinterpret_cast<int*>(ws) + ws_off : nullptr;
    if (p < G) ws_off += (size_t)ns[p] * 4;        // accumulators back to back; the counters follow the last one
  }
  // row blocks <= max_p ceil(n_p / 4) <= the counter words e8p_gemv_v2_workspace_words() reserves in total
  a.cnt = ws ? reinterpret_cast<int*>(ws) + ws_off : nullptr;
  a.grid = reinterpret_cast<const uint64_t*>(grid);
  a.K = k;
  a.kp_src = (k + 511) & ~511;
  a.segs = segs; a.spw = pl.spw; a.ksplit = pl.ksplit;
  a.dbg = reinterpret_cast<uint64_t*>(dbg);
  a.runlen = pl.runlen;
  a.rpr_inv = pl.rpr_inv;
}

}  // namespace quip
