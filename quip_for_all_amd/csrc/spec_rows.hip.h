// Speculative greedy decode, the bookkeeping between two chunk passes (part of decode_glue.hip's translation unit, behind
// nll_rows.hip.h, whose arg-max and log-sum-exp it reads): ACCEPT the guessed tokens the model confirmed, emit them and
// the model's own next token, take the position back behind them, and DRAFT the next guesses by prompt lookup -- the
// continuation of the most recent place where the last few tokens already occurred, in the caller's prediction or in the
// text itself.  DESIGN 4.18 holds the function; spec.py restates it on lists (accept_draft_ref).  One workgroup of
// kSpecThreads threads per launch: latency code, nothing here is wide.
//
// State (device; ids, pos, out_len, stats int64; n_draft, n_pred int32), n = k + 1 rows per pass:
//   rows_tok (n)   row 0 the current token, rows 1 .. n_draft guesses, 0 behind them
//   pos            arrives as p0 + n (the chunk loop advanced it); hist[p] is the token fed at position p, valid on
//                  [0, p0], hist[p0] == rows_tok[0]
//   pred (n_pred)  the caller's prediction;  out / out_len the emitted tokens;  stats = passes, drafted, accepted, status
//
// accept   d = n_draft;  a = the largest j in [0, d] with argmax[i] == rows_tok[i + 1] for all i < j and lse[i] finite
//          for all i <= j.  None (row 0 not finite): status |= 1, pos = p0, nothing else.  Else t = argmax[a]:
//          out += rows_tok[1 .. a], t (writes at or past cap_out are dropped, out_len counts them);  hist[p0 + 1 .. p0 + a]
//          = rows_tok[1 .. a], hist[p0 + a + 1] = t;  pos = p0 + a + 1;  stats += (1, d, a).
// draft    corpus C = pred[0 .. n_pred) ++ hist[0 .. pos], two segments.  A candidate is an end index e < len(C) - 1 whose
//          last m(e) tokens equal the last m(e) tokens of hist[0 .. pos], m(e) the longest such length <= gmax that stays
//          in e's segment and is <= pos + 1, if m(e) >= max(gmin, 1);  avail(e) = the tokens behind e in e's segment, >= 1
//          for every e < len(C) - 1 but the last one of pred.  The winner is the maximum of (m, min(avail, k), e) -- the
//          longest match, then the fullest continuation, then the most recent -- as ONE packed 64-bit key and one
//          max-reduction.  (Trying g = gmax down to gmin and taking the best (g, ., .) is the same thing: a match of
//          length g at e is a match of every shorter length.)  Guesses C[e + 1 .. e + min(avail, k)], n_draft their count,
//          rows_tok = [t, guesses, 0 ...].  A length of 0 is never a match: gmax = 0 turns drafting off.
//
// Inside the launch nothing is read from memory that the launch wrote: the tokens the accept step appends to hist are
// served from rows_tok (not yet rewritten) and from t (spec_hist), every thread picks up what it will write, then ONE
// barrier, then the stores.  State that cannot be right (a position outside hist) sets status |= 2 and writes nothing
// else.  LDS: the suffix (kSpecMaxG ids) and the kSpecThreads / 64 wave partials of the key.  No scratch, no atomics.
#pragma once
#include "launch.hip.h"
#include "quip_device.hip.h"

namespace quip {
namespace {

constexpr int kSpecThreads = 256;
constexpr int kSpecMaxK = 15;
constexpr int kSpecMaxG = 8;
constexpr int kSpecMaxCorpus = 1 << 20;
constexpr int kSpecLdsBytes = kSpecMaxG * 8 + (kSpecThreads / 64) * 8;

struct SpecState {
  int64_t* rows_tok;
  int32_t* n_draft;
  int64_t* pos;
  int64_t* hist;
  const int64_t* pred;
  const int32_t* n_pred;
  int64_t* stats;
  int hist_cap, pred_cap, k, gmin, gmax;
};

struct SpecShared {
  int64_t suffix[kSpecMaxG];                          // suffix[j] = hist[pos - j]
  unsigned long long part[kSpecThreads / 64];
};
static_assert(sizeof(SpecShared) == kSpecLdsBytes, "spec_rows.hip.h: the LDS figure of the header comment");

// hist[i] as it stands after the accept step, i <= p0 + a + 1: the stored part, the accepted guesses, the model's token
__device__ __forceinline__ int64_t spec_hist(const SpecState& st, int64_t i, int64_t p0, int a, int64_t t) {
  if (i <= p0) return st.hist[i];
  if (i <= p0 + a) return st.rows_tok[i - p0];
  return t;
}

// the accepted count a (-1: row 0 is not finite)
__device__ __forceinline__ int spec_accept(const int64_t* __restrict__ rows_tok, const int64_t* __restrict__ argmax,
                                           const float* __restrict__ lse, int d) {
  int a = -1;
  for (int j = 0; j <= d; ++j) {
    const float l = lse[j];
    if (!(l == l && l != INFINITY && l != -INFINITY)) break;
    if (j > 0 && argmax[j - 1] != rows_tok[j]) break;
    a = j;
  }
  return a;
}

// The winner's key over the corpus pred[0 .. np) ++ hist[0 .. pos] (hist through spec_hist), 0 without a candidate:
// match length << 40 | min(avail, k) << 32 | e.  Every thread returns the same key.
__device__ __forceinline__ unsigned long long spec_draft(const SpecState& st, SpecShared& sh, int np, int64_t pos, int64_t p0,
                                                         int a, int64_t t) {
  const int tid = threadIdx.x;
  const int len = np + (int)pos + 1;
  const int gcap = pos + 1 < st.gmax ? (int)(pos + 1) : st.gmax;
  const int glo = max(st.gmin, 1);
  if (tid < gcap) sh.suffix[tid] = spec_hist(st, pos - tid, p0, a, t);
  __syncthreads();
  unsigned long long best = 0;
  if (gcap >= glo) {
    for (int e = tid; e < len - 1; e += kSpecThreads) {
      const bool in_pred = e < np;
      const int s0 = in_pred ? 0 : np, s1 = in_pred ? np : len;
      const int avail = s1 - 1 - e;
      if (avail < 1) continue;
      const int mcap = min(gcap, e - s0 + 1);
      int m = 0;
      while (m < mcap) {
        const int i = e - m;
        const int64_t c = in_pred ? st.pred[i] : spec_hist(st, i - np, p0, a, t);
        if (c != sh.suffix[m]) break;
        ++m;
      }
      if (m >= glo) {
        const unsigned long long key = ((unsigned long long)m << 40) | ((unsigned long long)min(avail, st.k) << 32) | (unsigned)e;
        best = key > best ? key : best;           // (e ascends: a later candidate of the same rank wins)
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)best, o, 64), hi = __shfl_xor((unsigned)(best >> 32), o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    best = other > best ? other : best;
  }
  if ((tid & 63) == 0) sh.part[tid >> 6] = best;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < kSpecThreads / 64; ++w) best = sh.part[w] > best ? sh.part[w] : best;      // every thread: no broadcast
  return best;
}

// what thread `tid` <= k stores into rows_tok[tid] for the winner `key`: t, a guess, or 0; *c = the number of guesses
__device__ __forceinline__ int64_t spec_row(const SpecState& st, unsigned long long key, int np, int64_t p0, int a, int64_t t,
                                            int tid, int* c) {
  const int e = (int)(unsigned)key;
  *c = (int)((key >> 32) & 0xff);
  if (tid == 0) return t;
  if (tid > *c) return 0;
  const int i = e + tid;
  return i < np ? st.pred[i] : spec_hist(st, i - np, p0, a, t);
}

__device__ __forceinline__ void spec_flag(const SpecState& st, int bit) {
  if (threadIdx.x == 0) st.stats[3] |= bit;
}

__global__ __launch_bounds__(kSpecThreads) void spec_draft_kernel(SpecState st) {
  __shared__ SpecShared sh;
  const int tid = threadIdx.x;
  const int64_t pos = st.pos[0];
  if (pos < 0 || pos >= st.hist_cap) { spec_flag(st, 2); return; }
  const int np = min(max(st.n_pred[0], 0), st.pred_cap);
  const int64_t t = st.rows_tok[0];
  const unsigned long long key = spec_draft(st, sh, np, pos, pos, 0, t);
  int c = 0;
  const int64_t mine = tid <= st.k ? spec_row(st, key, np, pos, 0, t, tid, &c) : 0;
  __syncthreads();                                    // every read of rows_tok is behind us
  if (tid <= st.k) st.rows_tok[tid] = mine;
  if (tid == 0) st.n_draft[0] = c;
}

__global__ __launch_bounds__(kSpecThreads) void spec_accept_draft_kernel(SpecState st, const int64_t* __restrict__ argmax,
                                                                         const float* __restrict__ lse,
                                                                         int64_t* __restrict__ out,
                                                                         int64_t* __restrict__ out_len, int cap_out) {
  __shared__ SpecShared sh;
  const int tid = threadIdx.x;
  const int n = st.k + 1;
  const int64_t p0 = st.pos[0] - n;
  if (p0 < 0 || p0 + n >= st.hist_cap) { spec_flag(st, 2); return; }       // (hist[p0 + a + 1], a <= k, must exist)
  const int d = min(max(st.n_draft[0], 0), st.k);
  const int a = spec_accept(st.rows_tok, argmax, lse, d);
  if (a < 0) {
    __syncthreads();                                  // every thread has read pos
    if (tid == 0) { st.stats[3] |= 1; st.pos[0] = p0; }
    return;
  }
  const int64_t t = argmax[a];
  const int64_t pos = p0 + a + 1;
  const int np = min(max(st.n_pred[0], 0), st.pred_cap);
  const int64_t olen = out_len[0];
  const int64_t accepted = (tid >= 1 && tid <= a) ? st.rows_tok[tid] : t;   // thread j: rows_tok[j]; thread 0: t
  const unsigned long long key = spec_draft(st, sh, np, pos, p0, a, t);
  int c = 0;
  const int64_t mine = tid <= st.k ? spec_row(st, key, np, p0, a, t, tid, &c) : 0;
  __syncthreads();                                    // every read of rows_tok, pos, out_len is behind us
  if (tid <= a) {
    const int64_t at = tid == 0 ? a + 1 : tid;        // hist / out slot of this thread's token, counted from p0 / olen - 1
    st.hist[p0 + at] = accepted;
    const int64_t o = olen + at - 1;
    if (o >= 0 && o < cap_out) out[o] = accepted;
  }
  if (tid <= st.k) st.rows_tok[tid] = mine;
  if (tid == 0) {
    st.pos[0] = pos;
    st.n_draft[0] = c;
    out_len[0] = olen + a + 1;
    st.stats[0] += 1;
    st.stats[1] += d;
    st.stats[2] += a;
  }
}

int spec_check(const SpecState& st) {
  if (st.k < 1 || st.k > kSpecMaxK || st.gmin < 0 || st.gmin > st.gmax || st.gmax > kSpecMaxG || st.hist_cap < 1 ||
      st.pred_cap < 0 || (int64_t)st.hist_cap + st.pred_cap > kSpecMaxCorpus)
    return QUIP_ERR_BAD_SHAPE;
  return QUIP_OK;
}
}  // namespace

int spec_draft_launch(int64_t* rows_tok, int32_t* n_draft, int64_t* pos, int64_t* hist, int hist_cap, const int64_t* pred,
                      const int32_t* n_pred, int pred_cap, int64_t* stats, int k, int gmin, int gmax, hipStream_t stream) {
  const SpecState st{rows_tok, n_draft, pos, hist, pred, n_pred, stats, hist_cap, pred_cap, k, gmin, gmax};
  if (int rc = spec_check(st)) return rc;
  return launch<spec_draft_kernel>(dim3(1), dim3(kSpecThreads), 0, stream, st);
}

int spec_accept_draft_launch(const int64_t* argmax, const float* lse, int64_t* rows_tok, int32_t* n_draft, int64_t* pos,
                             int64_t* hist, int hist_cap, const int64_t* pred, const int32_t* n_pred, int pred_cap,
                             int64_t* out, int64_t* out_len, int cap_out, int64_t* stats, int k, int gmin, int gmax,
                             hipStream_t stream) {
  const SpecState st{rows_tok, n_draft, pos, hist, pred, n_pred, stats, hist_cap, pred_cap, k, gmin, gmax};
  if (int rc = spec_check(st)) return rc;
  if (cap_out < 0) return QUIP_ERR_BAD_SHAPE;
  return launch<spec_accept_draft_kernel>(dim3(1), dim3(kSpecThreads), 0, stream, st, argmax, lse, out, out_len, cap_out);
}

}  // namespace quip
