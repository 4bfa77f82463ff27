// nf_target_epilogue.h -- the target epilogue of the fused ELBO forwards (k_affine_chain_tgt of nf_coupling.hip,
// k_rqs_chain_tgt of nf_rqs.hip) for the built-in targets other than the diagonal Gaussian: log p(y_j) and
// ybar = gscale * grad log p(y) straight from the registers the last coupling left, through target_term (nf_targets.h) --
// the function k_target_tiled and nf_simple.hip evaluate, not a second transcription of the densities.  The NF_TGT_* sets of
// kinds (template argument KSET / TGT) are defined in nf_targets.h.
#pragma once
#include "nf_mfma.h"
#include "nf_targets.h"

// Register map of both chain kernels: E[b][r] is feature 2 * (b * 32 + nf_row(r, hi)) of sample l31, O[b][r] the one after
// it; features >= d and padding samples hold 0.  Features 0 and 1 therefore sit in E[0][0] / O[0][0] of the hi == 0
// half-wave; every other register is a feature >= 2, which is all target_term needs to know of its index.
//   y0, y1   read from lane l31 (one ds_bpermute each);
//   s2       (Funnel) sum_{i >= 1} y_i^2: the lane's partial plus the other half-wave's (a + b in both halves: same bits);
//   d = 2 kinds (WarpedGauss, Cross): only register (0, 0) of the hi == 0 half-wave is evaluated -- every other store would
//            fall beyond the tile's descriptor (d * 32 floats) anyway.
//   Banana, Funnel (d >= 2, nf_target_check): a feature i >= 2 that holds 0 contributes exactly 0 to log p and has gradient
//            0 (-v^2 / 2, -v; -a v^2 / 2, -a v), so the zero padding needs no mask -- thirty-two loop-invariant lane masks
//            would otherwise be hoisted out of the tile loop and held in scalar registers across the whole chain.
// A padding sample has y = 0, where WarpedGauss divides by r = 0: the stores SELECT (valid ? .. : 0), so no NaN reaches gt;
// the returned sum of such a lane is not used by the caller (contrib is taken for valid samples only).
// Returns log p(y_j), complete in both half-waves.
template <int KIND, int CB>
__device__ __forceinline__ float nf_tile_target_kind(const f32x16 (&E)[CB], const f32x16 (&O)[CB], int d, float s0, float s1, int l31,
                                                     int hi, const TileIO &gio, bool store, bool valid, float gscale) {
  constexpr bool D2 = KIND == NF_TARGET_WARPED || KIND == NF_TARGET_CROSS;
  const float y0 = __shfl(E[0][0], l31), y1 = __shfl(O[0][0], l31);
  float s2 = 0.f;
  if constexpr (KIND == NF_TARGET_FUNNEL) {
#pragma unroll
    for (int b = 0; b < CB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = E[b][r], o = O[b][r];
        s2 += ((b | r) == 0 && hi == 0 ? 0.f : e * e) + o * o;
      }
    s2 += __shfl_xor(s2, 32);
  }
  float t = 0.f;
#pragma unroll
  for (int b = 0; b < CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (D2 && (b | r) != 0) continue;
      const int fe = 2 * (b * 32 + nf_row(r, hi));  // the feature of E[b][r]
      const int ie = (b | r) == 0 ? fe : 2;         // what target_term distinguishes: 0, 1, anything else
      float ge, go;
      const float te = target_term<KIND, float>(d, ie, E[b][r], y0, y1, s2, nullptr, nullptr, s0, s1, ge);
      const float to = target_term<KIND, float>(d, ie + 1, O[b][r], y0, y1, s2, nullptr, nullptr, s0, s1, go);
      const bool in = D2 ? hi == 0 : true;  // (D2: the hi == 1 half-wave holds the zero padding of features 8, 9)
      t += in ? te + to : 0.f;
      if (store) {
        tile_store(gio, tile_soff(b, r, 0), valid && in ? gscale * ge : 0.f);
        tile_store(gio, tile_soff(b, r, 1), valid && in ? gscale * go : 0.f);
      }
    }
  t += __shfl_xor(t, 32);
  return t;
}

// Called by the chain bodies right before nf_tile_target: the tile's y passes through an opaque identity behind a scheduling
// barrier.  Without it hipcc schedules and allocates the last coupling's combine and the target arithmetic as one region, and
// the K = 8 spline kernel needs 255 registers + 20 bytes of scratch at two waves per SIMD whatever the epilogue computes; with
// it 242 and none (the diagonal-Gaussian kernel: 243).
template <int CB>
__device__ __forceinline__ void nf_tile_isolate(f32x16 (&E)[CB], f32x16 (&O)[CB]) {
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int b = 0; b < CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float e = E[b][r], o = O[b][r];
      asm volatile("" : "+v"(e), "+v"(o));
      E[b][r] = e;
      O[b][r] = o;
    }
}

// kind: wave-uniform (a kernel argument), one of the kinds in KSET -- the host launches nothing else here
template <int CB, int KSET>
__device__ __forceinline__ float nf_tile_target(int kind, const f32x16 (&E)[CB], const f32x16 (&O)[CB], int d, float s0, float s1,
                                                int l31, int hi, const TileIO &gio, bool store, bool valid, float gscale) {
  // The target's scalars and d are kernel arguments, so everything the densities derive from them alone (log s1, 1 / s0^2,
  // the Cross components' constants, ...) is invariant in the chain kernel's tile loop: hipcc hoists those values above the
  // loop and keeps them -- uniform, but in vector registers -- across every coupling, where the kernels are at their register
  // limit.  Made opaque here, they are computed where they are used.
  asm volatile("" : "+v"(s0), "+v"(s1), "+s"(d));
  if ((KSET & NF_TGT_BANANA) && (kind == NF_TARGET_BANANA || KSET == NF_TGT_BANANA))
    return nf_tile_target_kind<NF_TARGET_BANANA, CB>(E, O, d, s0, s1, l31, hi, gio, store, valid, gscale);
  if ((KSET & NF_TGT_FUNNEL) && (kind == NF_TARGET_FUNNEL || !(KSET & (NF_TGT_WARPED | NF_TGT_CROSS))))
    return nf_tile_target_kind<NF_TARGET_FUNNEL, CB>(E, O, d, s0, s1, l31, hi, gio, store, valid, gscale);
  if ((KSET & NF_TGT_WARPED) && (kind == NF_TARGET_WARPED || !(KSET & NF_TGT_CROSS)))
    return nf_tile_target_kind<NF_TARGET_WARPED, CB>(E, O, d, s0, s1, l31, hi, gio, store, valid, gscale);
  return nf_tile_target_kind<NF_TARGET_CROSS, CB>(E, O, d, s0, s1, l31, hi, gio, store, valid, gscale);
}
