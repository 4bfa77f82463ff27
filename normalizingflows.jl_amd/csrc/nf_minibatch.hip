// nf_minibatch.hip -- row-minibatch targets (gfx950): nf_target_minibatch builds, on the device and in one launch, a target of m
// rows out of a regression target's R rows IN THE FULL TARGET'S OWN KIND AND LAYOUT, so that every target kernel, every flow and
// every entry point serves it unchanged (it is a target with s0 = m).  Stochastic VI: resample before each step.
//
// Sampling rule (the specification; tests/minibatch_ref.py restates it in numpy): stratified, one row per stratum, without replacement.
//   lo_j  = floor(j R / m) (64-bit),  n_j = lo_{j+1} - lo_j >= 1                                j = 0 .. m-1
//   idx_j = lo_j + (((uint64) r_j * n_j) >> 32)
//   r_j   = word x of philox4x32_10(counter (j_lo, j_hi, 0xFFFFFFFF, stream), key (seed_lo, seed_hi))
// Counter word 2 = 0xFFFFFFFF is never a feature group of the base draws (nf_philox.h: groups are < 2^31 in Float32 and carry bit 31 over
// a small group index in Float64), so the row choice is disjoint from the draws even under the same seed and stream.
//   wt'_j = wt[idx_j] * (T) n_j  (one rounding), every other per-row value of row idx_j and every fixed segment verbatim.
// E[sum_j n_j wt_idx_j phi_idx_j] = sum_i wt_i phi_i: the estimator is unbiased; the host-folded full-data terms (lin, par, ctab) are
// copied and stay exact.  m = R gives idx_j = j, n_j = 1: the full target's buffers bit for bit.
//
// The layout is a table (MbTable): the segments of p0 in order, each per-row (length R in the source, m in the result) or fixed (its
// length), and the position of the weight segment.  The kernel takes the table, not the kind: another layout is a table row.
//
// k_minibatch_gather<T>: a workgroup owns MB_ROWS consecutive batch rows.  Lane r < MB_ROWS draws (or reads) idx of its row, bounds it by
// select to [0, R), writes idx_out and gathers the row's per-row values of p0; the workgroup then copies the rows of p1 -- 16-byte
// accesses when the row pitch and both bases allow, scalar accesses otherwise -- and all workgroups share the fixed segments.  Every
// output element has exactly one writer: no atomics, the same bits on every launch; row addresses are 64-bit.
#include "nf_common.h"
#include "nf_launchers.h"
#include "nf_philox.h"
#include "nf_targets.h"

#define MB_BLOCK 256
#define MB_ROWS 16     // batch rows per workgroup
#define MB_MAXSEG 16   // segments of the widest layout (the dispersion kinds: 13)

struct MbTable {
  int nseg;               // segments of p0, in order
  int wseg;               // which of them holds the row weights
  unsigned per_row;       // bit s: segment s has one element per row
  long len[MB_MAXSEG];    // length of a fixed segment (a per-row segment: R in the source, m in the result)
};

__host__ __device__ inline long mb_stratum_lo(long j, long R, long m) { return (long)(((unsigned long)j * (unsigned long)R) / (unsigned long)m); }

template <class T>
__global__ __launch_bounds__(MB_BLOCK) void k_minibatch_gather(MbTable tab, long R, long m, int w, int vec, uint32_t k0, uint32_t k1,
                                                               uint32_t stream, const int32_t *__restrict__ idx_in,
                                                               int32_t *__restrict__ idx_out, const T *__restrict__ p0,
                                                               const T *__restrict__ p1, T *__restrict__ p0_out, T *__restrict__ p1_out) {
  __shared__ int s_idx[MB_ROWS];
  const long j0 = (long)blockIdx.x * MB_ROWS;
  const int nrows = (int)(m - j0 < MB_ROWS ? m - j0 : MB_ROWS);
  if ((int)threadIdx.x < nrows) {
    const long j = j0 + threadIdx.x;
    const long lo = mb_stratum_lo(j, R, m);
    const long n = mb_stratum_lo(j + 1, R, m) - lo;
    long idx;
    if (idx_in) {
      idx = idx_in[j];
    } else {
      const U4 c = {(uint32_t)j, (uint32_t)((uint64_t)j >> 32), 0xFFFFFFFFu, stream};
      const U4 r = philox4x32_10(c, k0, k1);
      idx = lo + (long)(((uint64_t)r.x * (uint64_t)n) >> 32);
    }
    idx = idx < 0 ? 0 : (idx > R - 1 ? R - 1 : idx);  // bounded by select before it addresses anything
    s_idx[threadIdx.x] = (int)idx;
    if (idx_out) idx_out[j] = (int32_t)idx;
    long src = 0, dst = 0;
    for (int s = 0; s < tab.nseg; ++s) {
      if ((tab.per_row >> s) & 1u) {
        T v = p0[src + idx];
        if (s == tab.wseg) v = v * (T)n;
        p0_out[dst + j] = v;
        src += R;
        dst += m;
      } else {
        src += tab.len[s];
        dst += tab.len[s];
      }
    }
  }
  __syncthreads();
  if (vec) {  // w * sizeof(T) is a multiple of 16 and both bases are 16-byte aligned: so is every row
    const int vpr = (int)((size_t)w * sizeof(T) / 16);
    const uint4 *__restrict__ s4 = reinterpret_cast<const uint4 *>(p1);
    uint4 *__restrict__ d4 = reinterpret_cast<uint4 *>(p1_out);
    for (int t = threadIdx.x; t < nrows * vpr; t += MB_BLOCK) {
      const int r = t / vpr, c = t - r * vpr;
      d4[(j0 + r) * vpr + c] = s4[(long)s_idx[r] * vpr + c];
    }
  } else {
    for (int t = threadIdx.x; t < nrows * w; t += MB_BLOCK) {
      const int r = t / w, c = t - r * w;
      p1_out[(j0 + r) * w + c] = p1[(long)s_idx[r] * w + c];
    }
  }
  // the fixed segments, shared by all workgroups
  const long gsz = (long)gridDim.x * MB_BLOCK, gid = (long)blockIdx.x * MB_BLOCK + threadIdx.x;
  long src = 0, dst = 0;
  for (int s = 0; s < tab.nseg; ++s) {
    if ((tab.per_row >> s) & 1u) {
      src += R;
      dst += m;
    } else {
      const long len = tab.len[s];
      for (long e = gid; e < len; e += gsz) p0_out[dst + e] = p0[src + e];
      src += len;
      dst += len;
    }
  }
}

// The segment table of a kind at (d, s1), with the table length of the negative-binomial kind left at 0, and the row width w of p1.
// false: the kind has no per-row weight, or its rows are not exchangeable.
static bool mb_layout(const nf_target *t, int d, MbTable *tab, int *w) {
  const int kind = t->kind;
  int n = 0;
  tab->per_row = 0;
  auto fixed = [&](long len) { tab->len[n++] = len; };
  auto rows = [&](bool weight = false) {
    if (weight) tab->wseg = n;
    tab->per_row |= 1u << n;
    tab->len[n++] = 0;
  };
  if (target_is_glm(kind)) {  // lin[d] | off | wt | par[2]
    fixed(d), rows(), rows(true), fixed(2);
    *w = d;
  } else if (target_is_hglm(kind)) {  // lin[d] | off | wt | par[2] | grp[p] | isd[p] | hm[G] | his[G] | hk[G] | gptr[G + 1] | gidx[p]
    const int G = (int)t->s1, p = d - G;
    fixed(d), rows(), rows(true), fixed(2), fixed(p), fixed(p), fixed(G), fixed(G), fixed(G), fixed(G + 1), fixed(p);
    *w = d;
  } else if (target_is_dglm(kind)) {  // lin[d] | off | wt | par[4] | grp[p] | isd[p] | hm, his, hk, gptr [G + 1] | gidx[p] ( | cnt | ctab[Mt])
    const int G = (int)t->s1, p = d - G - 1;
    fixed(d), rows(), rows(true), fixed(4), fixed(p), fixed(p), fixed(G + 1), fixed(G + 1), fixed(G + 1), fixed(G + 1), fixed(p);
    if (kind == NF_TARGET_DGLM_NEGBIN) rows(), fixed(0);
    *w = d;
  } else if (kind == NF_TARGET_SOFTMAX) {  // lab | wt | par[2]
    rows(), rows(true), fixed(2);
    *w = d / (int)t->s1;
  } else if (target_is_bnn(kind)) {  // scl | off | wt | par[4]
    rows(), rows(), rows(true), fixed(4);
    *w = (d - 1) / (int)t->s1 - 1;
  } else {
    return false;
  }
  tab->nseg = n;
  return true;
}

extern "C" int nf_target_minibatch(nf_ctx *ctx, int32_t dtype, const nf_target *full, int32_t d, int64_t p0_elems, int64_t m,
                                   uint64_t mb_seed, uint32_t stream, const int32_t *idx_in, int32_t *idx_out, void *p0_out,
                                   void *p1_out, nf_target *out) {
  if (!ctx || !full || !out || !p0_out || !p1_out || d < 1) return NF_ERR_ARG;
  if (dtype != NF_DTYPE_F32 && dtype != NF_DTYPE_F64) return NF_ERR_ARG;
  const int kind = full->kind;
  if ((kind >= NF_TARGET_DIAGGAUSS && kind <= NF_TARGET_LOGREG) || kind == NF_TARGET_GAUSSMIX || target_is_ordinal(kind) ||
      target_is_riskset(kind))
    return NF_ERR_UNSUPPORTED;  // no per-row weight (0 .. 6, 8), rows grouped by label blocks (32), rows that interact (33)
  NF_TRY(nf_target_check(full, d));  // NULL p0 / p1, s0, s1, d: the kind's own conventions (unassigned kinds: NF_ERR_ARG)
  MbTable tab;
  int w = 0;
  if (!mb_layout(full, d, &tab, &w)) return NF_ERR_UNSUPPORTED;
  const long R = (long)full->s0;
  if (m < 1 || m > R || p0_out == full->p0 || p1_out == full->p1 || w < 1) return NF_ERR_ARG;
  long need = 0;
  for (int s = 0; s < tab.nseg; ++s) need += ((tab.per_row >> s) & 1u) ? R : tab.len[s];
  if (kind == NF_TARGET_DGLM_NEGBIN) {  // the table length lives in device memory: it is what p0_elems leaves (the kernels' bound: 4096)
    const long Mt = (long)p0_elems - need;
    if (Mt < 0 || Mt > 4096) return NF_ERR_ARG;
    tab.len[tab.nseg - 1] = Mt;
  } else if ((long)p0_elems != need) {
    return NF_ERR_ARG;
  }
  NF_HIP(hipSetDevice(ctx->device));
  const size_t es = dtype == NF_DTYPE_F32 ? 4 : 8;
  const int vec = ((size_t)w * es) % 16 == 0 && ((uintptr_t)full->p1 & 15) == 0 && ((uintptr_t)p1_out & 15) == 0;
  const dim3 grid((unsigned)((m + MB_ROWS - 1) / MB_ROWS)), block(MB_BLOCK);
  const uint32_t k0 = (uint32_t)mb_seed, k1 = (uint32_t)(mb_seed >> 32);
  {
    ProfScope ps(ctx, "target_minibatch");
    if (dtype == NF_DTYPE_F32)
      hipLaunchKernelGGL(k_minibatch_gather<float>, grid, block, 0, ctx->stream, tab, R, (long)m, w, vec, k0, k1, stream, idx_in, idx_out,
                         (const float *)full->p0, (const float *)full->p1, (float *)p0_out, (float *)p1_out);
    else
      hipLaunchKernelGGL(k_minibatch_gather<double>, grid, block, 0, ctx->stream, tab, R, (long)m, w, vec, k0, k1, stream, idx_in, idx_out,
                         (const double *)full->p0, (const double *)full->p1, (double *)p0_out, (double *)p1_out);
  }
  NF_HIP(hipGetLastError());
  out->kind = kind;
  out->p0 = p0_out;
  out->p1 = p1_out;
  out->s0 = (double)m;
  out->s1 = full->s1;
  return NF_OK;
}
