// nf_coupling.hip -- AffineCoupling (RealNVP) kernels for gfx950.
//
// Reference arithmetic: src/flows/realnvp.jl:57-110
//   forward  y1 = x1 .* exp.(s(x2)) .+ t(x2),  logjac =  sum(s(x2); dims=1)
//   inverse  x1 = (y1 .- t(y2)) .* exp.(-s(y2)), logjac = -sum(s(y2); dims=1)
// with s, t = fnn(...) (src/flows/utils.jl:71-100; s ends in tanh, realnvp.jl:50).
// PartitionMask partition/combine (realnvp.jl:59,62) is index arithmetic in the loads
// and stores here: transformed feature p <-> 2p + par_t, conditioner q <-> 2q + 1 - par_t.
//
// Work decomposition: one wavefront = one tile of 32 samples, activations chained through
// the fp32 matrix pipe in registers (nf_mfma.h); weights of the coupling live in LDS.
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "nf_common.h"
#include "nf_launchers.h"
#include "nf_mfma.h"
#include "nf_pack.h"
#include "nf_philox.h"
#include "nf_target_epilogue.h"

struct CouplingArgs {
  const float *theta;
  const float *img_s, *img_t;  // pre-packed LDS images of the s / t nets (k_pack_net_images)
  long long *trace;            // optional s_memtime stamps of block 0 / wave 0 (nf_debug_trace)
  NetDims s, t;
  int d, c, m, par_t;
  long N;
};

// ------------------------------------------------------------------------------------
// whole-flow forward / inverse in ONE launch (with_logabsdet_jacobian of the ComposedFunction,
// reached from src/objectives/elbo.jl:67; inverse chain from loglikelihood.jl:31)
// ------------------------------------------------------------------------------------
// A workgroup (8 waves) takes a group of 8 tiles through every coupling.  The state of a tile
// lives in registers for the whole chain, split by feature parity: E = features 0,2,4,..
// (transformed by the 1:2:d couplings), O = features 1,3,5,.. (transformed by the 2:2:d ones),
// so "partition/combine" is just which of the two register blocks plays x1 and which x2.
// The two nets of the NEXT coupling are fetched from their packed images (L2) while the current
// coupling computes, into the other half of a double-buffered LDS image.
struct ChainArgs {
  const float *wimg;  // [coupling][s|t][G::SIZE] packed images
  const unsigned char *wimg_b6;  // [coupling][s|t][B6Geo<G>::BYTES]: the same weights as bf16 triples (B6 kernels)
  int d, ncoup;
  long N;
};

// the conditioner net on the bf16 matrix cores (nf_mfma.h "B6"): same layers, the image is a B6Geo<G> image
// PIPE: the layers as software pipelines (dense_fwd_b6p); false: the plain form, 44 registers less (three waves per SIMD)
template <class G, bool PIPE = true>
__device__ __forceinline__ void net_forward_b6(const float *__restrict__ img, const f32x16 (&x)[G::MB], f32x16 (&out)[G::CB],
                                               int l31, int hi) {
  using B = B6Geo<G>;
  const nf_u32x4 *w = reinterpret_cast<const nf_u32x4 *>(img);
  const float *bias = reinterpret_cast<const float *>(w + B::BIAS);
  f32x16 a1[G::H1B], a2[G::H2B];
  if constexpr (PIPE) {  // the leaky ReLUs inside the next layer's splits (dense_fwd_b6p<..., LRIN>): same values, same bits
    dense_fwd_b6p<G::MB, G::H1B>(w + B::L1, bias + B::B1, x, a1, l31, hi);
    dense_fwd_b6p<G::H1B, G::H2B, true>(w + B::L2, bias + B::B2, a1, a2, l31, hi);
    dense_fwd_b6p<G::H2B, G::CB, true>(w + B::L3, bias + B::B3, a2, out, l31, hi);
  } else {
    dense_fwd_b6<G::MB, G::H1B>(w + B::L1, bias + B::B1, x, a1, l31, hi);
#pragma unroll
    for (int b = 0; b < G::H1B; ++b) nf_lrelu16(a1[b]);
    dense_fwd_b6<G::H1B, G::H2B>(w + B::L2, bias + B::B2, a1, a2, l31, hi);
#pragma unroll
    for (int b = 0; b < G::H2B; ++b) nf_lrelu16(a2[b]);
    dense_fwd_b6<G::H2B, G::CB>(w + B::L3, bias + B::B3, a2, out, l31, hi);
  }
}

struct NoBetween {
  __device__ __forceinline__ void operator()() const {}
};
// B6: img_s / img_t are B6 images; `between` runs between the two nets (the B6 chain kernel's image rotation: a workgroup
// barrier and the request for the image after next)
template <class G, bool INVERSE, bool B6 = false, class BT = NoBetween, bool PIPE = true>
__device__ __forceinline__ float coupling_step(const float *__restrict__ img_s, const float *__restrict__ img_t,
                                               f32x16 (&x1)[G::CB], const f32x16 (&xb)[G::MB], int l31, int hi, BT between = BT(),
                                               long long *tr = nullptr) {
  f32x16 S[G::CB], T[G::CB];
  if constexpr (B6) {
    NF_STAMP(tr, 0);  // tools/trace_chain.py (NOSTASH=1): after the phase barrier + the request for the image after next
    net_forward_b6<G, PIPE>(img_s, xb, S, l31, hi);
    NF_STAMP(tr, 1);
    between();
    NF_STAMP(tr, 2);
    net_forward_b6<G, PIPE>(img_t, xb, T, l31, hi);
    NF_STAMP(tr, 3);
  } else {
  {
    f32x16 a1[G::H1B], a2[G::H2B];
    net_forward<G>(img_s, xb, a1, a2, S, l31, hi);
  }
  between();
  {
    f32x16 a1[G::H1B], a2[G::H2B];
    net_forward<G>(img_t, xb, a1, a2, T, l31, hi);
  }
  }
  float lsum = 0.f;
#pragma unroll
  for (int b = 0; b < G::CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      // rows >= c have zero weights and biases in the packed image: s = 0, T = 0, x1 stays 0
      const float s = nf_tanh(S[b][r]);
      if (INVERSE)
        x1[b][r] = nf_fdiv(x1[b][r] - T[b][r], nf_exp(s));
      else
        x1[b][r] = x1[b][r] * nf_exp(s) + T[b][r];
      {
        // no contraction with nf_tanh's last product: whether hipcc fuses it into this sum differs from one kernel this function is
        // inlined into to the next (seen: k_affine_chain against k_affine_apply_b6 at hidden 64, ladj one ulp apart with bit-equal y),
        // and a chain of single couplings must add up to the whole chain bit for bit
#pragma clang fp contract(off)
        lsum += s;
      }
    }
  return lsum;
}

// ------------------------------------------------------------------------------------
// forward / inverse of one coupling (no gradients): both nets resident in LDS
// ------------------------------------------------------------------------------------
template <class G, bool INVERSE, bool FULL>
__global__ __launch_bounds__(512) void k_affine_apply(CouplingArgs a, const float *x_in,
                                                      float *y_out, float *__restrict__ ladj,
                                                      int ladj_accumulate) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *img_s = lds;
  float *img_t = lds + G::SIZE;
  const int tid = threadIdx.x;
  stage_packed<G::SIZE, 512>(img_s, a.img_s, tid);
  stage_packed<G::SIZE, 512>(img_t, a.img_t, tid);
  __syncthreads();

  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform
  const int l31 = lane & 31, hi = lane >> 5;
  const int par_c = 1 - a.par_t;
  const long ntiles = (a.N + NF_TILE - 1) / NF_TILE;
  const bool copy_cond = (y_out != x_in);

  for (long tile = (long)blockIdx.x * 8 + wave; tile < ntiles; tile += (long)gridDim.x * 8) {
    const long j = tile * NF_TILE + l31;
    const bool valid = FULL ? true : j < a.N;
    const TileIO xin = make_tile_io(const_cast<float *>(x_in), tile, a.d, l31, hi);
    const TileIO yout = make_tile_io(y_out, tile, a.d, l31, hi);

    f32x16 xb[G::MB], x1[G::CB];
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = tile_load(xin, tile_soff(b, r, par_c));
        xb[b][r] = valid ? v : 0.f;
        if (copy_cond) tile_store(yout, tile_soff(b, r, par_c), v);
      }
#pragma unroll
    for (int b = 0; b < G::CB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) x1[b][r] = tile_load(xin, tile_soff(b, r, a.par_t));

    // the coupling itself is the whole-chain kernel's coupling_step (k_affine_chain's fp32 form runs the same function on the same
    // images), so that under NF_FWD_FP32 too a chain of single couplings is the whole chain bit for bit; rows >= c have zero
    // weights and biases in the packed image: s = 0, t = 0
    float lsum = coupling_step<G, INVERSE>(img_s, img_t, x1, xb, l31, hi);
#pragma unroll
    for (int b = 0; b < G::CB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) tile_store(yout, tile_soff(b, r, a.par_t), x1[b][r]);  // rows >= c are outside the descriptor
    lsum += __shfl_xor(lsum, 32);
    if (hi == 0 && valid) {
      const float base = ladj_accumulate ? ladj[j] : 0.f;
      ladj[j] = INVERSE ? base - lsum : base + lsum;
    }
  }
}

// One coupling in place on the tiled buffer with the arithmetic of the whole-chain kernel (k_affine_chain's B6 form: the same
// coupling_step on the same bf16-triple images, the same fold of the log-determinant), so that nf_layer_apply of every coupling,
// chained, IS nf_flow_fwd / nf_flow_inv bit for bit.  img6: the coupling's s and t B6 images, adjacent.
template <class G, bool INVERSE>
__global__ __launch_bounds__(512) void k_affine_apply_b6(CouplingArgs a, const unsigned char *__restrict__ img6, float *xy,
                                                         float *__restrict__ ladj, int ladj_accumulate) {
  using BG = B6Geo<G>;
  static_assert(BG::BYTES % 16 == 0, "B6 images are copied in 16-byte pieces");
  constexpr int B6F = BG::BYTES / 4;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  stage_packed<2 * B6F, 512>(lds, reinterpret_cast<const float *>(img6), tid);
  __syncthreads();
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const int par_c = 1 - a.par_t;
  const long ntiles = (a.N + NF_TILE - 1) / NF_TILE;
  for (long tile = (long)blockIdx.x * 8 + wave; tile < ntiles; tile += (long)gridDim.x * 8) {
    const long j = tile * NF_TILE + l31;
    const bool valid = j < a.N;
    const TileIO io = make_tile_io(xy, tile, a.d, l31, hi);
    f32x16 xb[G::MB], x1[G::CB];
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = tile_load(io, tile_soff(b, r, par_c));  // features >= d read as 0
        xb[b][r] = valid ? v : 0.f;
      }
#pragma unroll
    for (int b = 0; b < G::CB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = tile_load(io, tile_soff(b, r, a.par_t));
        x1[b][r] = valid ? v : 0.f;
      }
    float ls = coupling_step<G, INVERSE, true>(lds, lds + B6F, x1, xb, l31, hi);
#pragma unroll
    for (int b = 0; b < G::CB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) tile_store(io, tile_soff(b, r, a.par_t), x1[b][r]);  // rows >= c are outside the descriptor
    ls += __shfl_xor(ls, 32);
    if (hi == 0 && valid) {
      const float base = ladj_accumulate ? ladj[j] : 0.f;
      ladj[j] = INVERSE ? base - ls : base + ls;
    }
  }
}

// ---- activation stash of the training step (forward writes, reverse pass reads) ---------------------------
// The reverse pass needs, per (tile, coupling): the conditioner input x2, both nets' hidden activations a1 / a2 and
// their leaky-ReLU sign masks, s = tanh(.) and u = x1 exp(s).  Recomputing them (k_affine_bwd_all) costs a third of
// that kernel's MFMAs plus the activations' LDS transposes; with STASH the fused forward writes them once, in the
// layouts the reverse pass consumes directly:
//   "T layout" (x2, a1, a2 -- the dW operands): [feature 32][sample parity 2][16] per 32-feature block, so the lane
//     that owns feature f in the dW GEMM reads its 16 k-steps (samples 2t + parity) as four 16-byte loads;
//   "lane layout" (s, u, masks -- element-wise operands in the MFMA C layout): [lane 64][16] per block.
// 46 KiB per (tile, coupling) for d = 64 / hidden 64: 772 MB per step at cfg 2.
// UV is WRITTEN AND READ FOR FLAT COUPLING ncoup - 1 ONLY, and holds x1 there (u = x1 exp(s) is one multiply by the exp(s) that
// phase S of the reverse pass evaluates anyway; the inverse direction's w1 as before).  The couplings alternate halves, so the
// half that flat coupling k transforms is the half that flat coupling k + 1 conditions on, and k + 1's slot has it as XT, stored
// from the same registers -- the same bits.  Which slot, in both directions: the forward chain applies flat coupling ncoup - 1
// first (coupling_at(s) = ncoup - 1 - s), so k's x1 is what k + 1, applied just before it, passed through; the inverse chain
// applies coupling 0 first (coupling_at(s) = s), so k's output w1 is what k + 1, applied just after it, reads.  Either way the
// neighbour of slot k is slot k + 1, and flat coupling ncoup - 1 (position 0 of the forward chain, the last position of the
// inverse chain) has none and keeps UV.  For every other coupling the UV region of the slot stays unwritten and unread: the
// slot keeps its size and layout, 42 KiB of the 46 are written (hidden 64), 713 MB per step at cfg 2, written once and read once.
// SLIM (round 4; optional, NF_STASH_SLIM=1 -- see stash_slim() for the measurement that keeps it off): WITHOUT a1.  The first hidden layer's activations are 35 %
// of the full stash (128 of 368 floats per sample and coupling) and the cheapest thing in it to rebuild: the consumer wave
// recomputes a1^T = leakyrelu(W1 x2 + b1) from x2 -- kept a second time in the MFMA C layout (XL), which is the A operand
// of that product -- with 32 MFMAs per net and tile while the producer wave is in its MFMA-free prologue.  34 KiB instead
// of 46 KiB per (tile, coupling): 570 instead of 772 MB per cfg-2 step, written once and read once.
template <class G, bool SLIM = false>
struct StashGeo {
  static constexpr int XT = 0;
  static constexpr int XL = XT + G::MB * 1024;  // SLIM only: x2 in the C ("lane") layout
  static constexpr int SV = XL + (SLIM ? G::MB * 1024 : 0);
  static constexpr int UV = SV + G::CB * 1024;
  static constexpr int NET0 = UV + G::CB * 1024;  // net 0 = s, net 1 = t
  static constexpr int A1 = 0, A2 = SLIM ? 0 : G::H1B * 1024, MSK = A2 + G::H2B * 1024, NETSZ = MSK + 256;
  static constexpr int SIZE = NET0 + 2 * NETSZ;  // floats per (tile, coupling), a multiple of 4
};
// Store instructions a wave of the stashing forward issues per phase (= per net) of a coupling that does NOT keep UV: the s
// net's phase stores x2 (element stores; SLIM: also XL, 16-byte stores), a1 and a2 (element stores) and the mask word, the t
// net's phase a1, a2, the mask word and s.  affine_chain_body's phase barrier counts on them (its comment).
//                      S_NET   T_NET   sum
//   hidden 64            81      69    150   (73 with UV)
//   hidden 32            49      37     86
//   hidden 64, SLIM      53      37     90
template <class G, bool SLIM>
struct StashStores {
  static constexpr int ACT = (SLIM ? 0 : G::H1B * 16) + G::H2B * 16 + 1;
  static constexpr int S_NET = G::MB * 16 + (SLIM ? G::MB * 4 : 0) + ACT;
  static constexpr int T_NET = ACT + G::CB * 4;
};
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// A buffer store of more than 64 bits must not be followed directly by a VALU write of its data registers.  hipcc's hazard
// recognizer inserts the wait state only when the instruction's soffset is NOT an SGPR (the ISA manual exempts the SGPR
// form).  Measured on MI355X, the SGPR form races as well: in k_affine_chain<hidden 32, FUSED, STASH> the mask store was
// followed by `v_add_u32` into its first data register, and lanes 12-15 of every 16-lane row of that word arrived in
// memory as the sum -- an LDS address -- in most runs with 8 live waves per workgroup (tools/kernel_resources.py,
// DESIGN.md section 5).  So wide stores pass their whole offset through the VGPR / immediate fields and soffset = 0, which
// puts them under the compiler's own guard.
__device__ __forceinline__ void nf_buffer_store_b128(u32x4 v, __amdgpu_buffer_rsrc_t rs, int voff, int coff) {
  __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff + coff, 0, 0);
}
struct StashIO {
  __amdgpu_buffer_rsrc_t rs;
  int vT, vL;  // per-lane byte offsets: T-layout element stores (C-layout lane), lane-layout rows
};
// live = false: a descriptor of extent 0, every store is dropped (idle waves of the last tile group)
__device__ __forceinline__ StashIO make_stash_io(float *stash, long slot, int size, bool live, int l31, int hi) {
  StashIO st;
  st.rs = __builtin_amdgcn_make_buffer_rsrc(stash + slot * size, 0, live ? size * 4 : 0, 0x00020000);
  st.vT = ((4 * hi) * 32 + (l31 & 1) * 16 + (l31 >> 1)) * 4;
  st.vL = (hi * 32 + l31) * 64;
  return st;
}
// element e (= block * 16 + reg) of a C-layout array into its T-layout slot
template <int NB>
__device__ __forceinline__ void stash_put_T(const StashIO &st, int base, const f32x16 (&v)[NB], int e) {
  if (e < NB * 16) {
    const int r = e & 15;
    const float val = v[e >> 4][r];  // (bit_cast straight on a vector element reads element 0 under hipcc 7.2)
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), st.rs, st.vT,
                                          (base + ((e >> 4) * 32 + (r & 3) + 8 * (r >> 2)) * 32) * 4, 0);
  }
}
template <int NB>
__device__ __forceinline__ void stash_put_lane(const StashIO &st, int base, const f32x16 (&v)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float val = v[b][4 * q + e];
        w[e] = __builtin_bit_cast(unsigned, val);
      }
      nf_buffer_store_b128(w, st.rs, st.vL, (base + b * 1024) * 4 + q * 16);
    }
}

// The masks the stashing forward leaves for the reverse pass.  DEVIATION, hidden-64 geometry only (NetGeo<1, 2, 2, 1>: the forward
// whose stash k_affine_bwd_pair reads -- bench.py's step): the mask is the activation's SIGN BIT, so a pre-activation of
// exactly +0 differentiates with slope 1 where the reference and every other kernel here use 0.01.  nf_sign_mask16's exact
// rule costs one more vector instruction per element in a kernel that is issue-bound: measured on one MI355X in three
// alternating runs, 0.5558 / 0.5596 / 0.5617 ms per step against the parent's 0.5517 / 0.5484 / 0.5478 (+1.8 %, the parent's
// own spread: 0.7 %; DESIGN sections 4 and 5).  A unit with all-zero weights and bias, or a conditioner half of exactly 0,
// gets db / dW rows 100 x the reference's on this path; nf_ctx_set_stash_budget(0) (the recompute pass) is exact.
template <class G>
__device__ __forceinline__ unsigned stash_mask16(const f32x16 &v) {
  if constexpr (G::H1B == 2 && G::H2B == 2) {
    unsigned bits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) bits = __builtin_amdgcn_alignbit(bits, (unsigned)__float_as_int(v[r]), 31);
    asm volatile("" : "+v"(bits));
    return bits;
  } else {
    return nf_sign_mask16(v);
  }
}

template <class G, bool STORE_X, bool SLIM = false, bool B6 = false>
__device__ __forceinline__ void net_forward_stash(const float *__restrict__ img, const f32x16 (&x)[G::MB], f32x16 (&out)[G::CB],
                                                  int l31, int hi, const StashIO &st, int nbase) {
  using SG = StashGeo<G, SLIM>;
  f32x16 a1[G::H1B], a2[G::H2B];
  unsigned m1[2] = {0u, 0u}, m2[2] = {0u, 0u};
  if constexpr (B6) {  // the same stores ride on the bf16 product's (fewer) MFMAs: two side-job slots per instruction
    using B = B6Geo<G>;
    const nf_u32x4 *w = reinterpret_cast<const nf_u32x4 *>(img);
    const float *bias = reinterpret_cast<const float *>(w + B::BIAS);
    auto sjx = [&](int e) { stash_put_T<G::MB>(st, SG::XT, x, e); };
    auto sj1 = [&](int e) { stash_put_T<G::H1B>(st, nbase + SG::A1, a1, e); };
    auto sj2 = [&](int e) { stash_put_T<G::H2B>(st, nbase + SG::A2, a2, e); };
    if (STORE_X) {
      if (SLIM) stash_put_lane<G::MB>(st, SG::XL, x);
      dense_fwd_b6<G::MB, G::H1B, decltype(sjx), true>(w + B::L1, bias + B::B1, x, a1, l31, hi, sjx);
    } else
      dense_fwd_b6<G::MB, G::H1B, NoSideJob, true>(w + B::L1, bias + B::B1, x, a1, l31, hi);
#pragma unroll
    for (int b = 0; b < G::H1B; ++b) {
      nf_lrelu16(a1[b]);
      m1[b] = stash_mask16<G>(a1[b]);
    }
    if (SLIM)
      dense_fwd_b6<G::H1B, G::H2B, NoSideJob, true>(w + B::L2, bias + B::B2, a1, a2, l31, hi);
    else
      dense_fwd_b6<G::H1B, G::H2B, decltype(sj1), true>(w + B::L2, bias + B::B2, a1, a2, l31, hi, sj1);
#pragma unroll
    for (int b = 0; b < G::H2B; ++b) {
      nf_lrelu16(a2[b]);
      m2[b] = stash_mask16<G>(a2[b]);
    }
    dense_fwd_b6<G::H2B, G::CB, decltype(sj2), true>(w + B::L3, bias + B::B3, a2, out, l31, hi, sj2);
    const u32x4 mkb = {m1[0], m1[1], m2[0], m2[1]};
    nf_buffer_store_b128(mkb, st.rs, (hi * 32 + l31) * 16, (nbase + SG::MSK) * 4);
    return;
  }
  if (STORE_X) {
    if (SLIM) stash_put_lane<G::MB>(st, SG::XL, x);
    dense_fwd<G::MB, G::H1B>(img + G::W1, img + G::B1, x, a1, l31, hi, [&](int e) { stash_put_T<G::MB>(st, SG::XT, x, e); });
  } else
    dense_fwd<G::MB, G::H1B>(img + G::W1, img + G::B1, x, a1, l31, hi);
#pragma unroll
  for (int b = 0; b < G::H1B; ++b) {
    nf_lrelu16(a1[b]);
    m1[b] = stash_mask16<G>(a1[b]);
  }
  if (SLIM)
    dense_fwd<G::H1B, G::H2B>(img + G::W2, img + G::B2, a1, a2, l31, hi);
  else
    dense_fwd<G::H1B, G::H2B>(img + G::W2, img + G::B2, a1, a2, l31, hi,
                              [&](int e) { stash_put_T<G::H1B>(st, nbase + SG::A1, a1, e); });
#pragma unroll
  for (int b = 0; b < G::H2B; ++b) {
    nf_lrelu16(a2[b]);
    m2[b] = stash_mask16<G>(a2[b]);
  }
  dense_fwd<G::H2B, G::CB>(img + G::W3, img + G::B3, a2, out, l31, hi,
                           [&](int e) { stash_put_T<G::H2B>(st, nbase + SG::A2, a2, e); });
  const u32x4 mk = {m1[0], m1[1], m2[0], m2[1]};
  nf_buffer_store_b128(mk, st.rs, (hi * 32 + l31) * 16, (nbase + SG::MSK) * 4);
}

// forward coupling of the training step: as coupling_step<G, false>, leaving the reverse pass's operands behind
// INVERSE (forward-KL training: the chain runs data -> base): w1 = (v1 - t) exp(-s); the UV slot then holds w1, which is
// what the reverse pass of the inverse coupling needs next to s (bwd_tile's INVD algebra)
// keep_uv: this is flat coupling ncoup - 1, the only one whose UV region is written (x1, or w1 under INVERSE) -- every other
// coupling's reverse pass takes the value from slot k + 1's XT (the comment above StashGeo)
// YFMA (forward direction): the output x1 exp(s) + t as ONE fma; otherwise the rounded product, then the sum.  While u was
// stored, the product had a second use and hipcc contracted the sum at one of the chain loop's two call sites only, the one
// of the even flat couplings (x1 = E), in every stashing instantiation.  The call sites name that choice, so that the flow
// output keeps its bits whatever the compiler would choose now.
template <class G, bool INVERSE = false, bool SLIM = false, bool B6 = false, bool YFMA = false, class BT = NoBetween>
__device__ __forceinline__ float coupling_step_stash(const float *__restrict__ img_s, const float *__restrict__ img_t,
                                                     f32x16 (&x1)[G::CB], const f32x16 (&xb)[G::MB], int l31, int hi,
                                                     const StashIO &st, bool keep_uv, long long *tr = nullptr, BT between = BT()) {
  using SG = StashGeo<G, SLIM>;
  static_assert(G::H1B <= 2 && G::H2B <= 2, "mask words");
  static_assert(G::MB == G::CB, "a neighbour's XT stands in for UV: both halves have the same padded size");
  f32x16 S[G::CB], T[G::CB];
  net_forward_stash<G, true, SLIM, B6>(img_s, xb, S, l31, hi, st, SG::NET0);
  NF_STAMP(tr, 1);
  between();
  net_forward_stash<G, false, SLIM, B6>(img_t, xb, T, l31, hi, st, SG::NET0 + SG::NETSZ);
  NF_STAMP(tr, 2);
  float lsum = 0.f;
#pragma unroll
  for (int b = 0; b < G::CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float s = nf_tanh(S[b][r]);
      if (INVERSE) {
        const float w = nf_fdiv(x1[b][r] - T[b][r], nf_exp(s));
        x1[b][r] = w;
        T[b][r] = w;
      } else {
#pragma clang fp contract(off)  // (YFMA, above: the contraction is stated, not left to the compiler)
        const float x = x1[b][r], e = nf_exp(s);
        x1[b][r] = YFMA ? __builtin_fmaf(x, e, T[b][r]) : x * e + T[b][r];
        T[b][r] = x;  // the reverse pass forms u = x e itself
      }
      S[b][r] = s;
      lsum += s;
    }
  stash_put_lane<G::CB>(st, SG::SV, S);
  if (keep_uv) stash_put_lane<G::CB>(st, SG::UV, T);  // wave-uniform: only flat coupling ncoup - 1 has no neighbour (StashGeo)
  return lsum;
}

// FUSED (forward only): the ELBO forward of the training step in the same launch -- the tile's base
// draws are generated in registers (Philox4x32-10 + Box-Muller, same counters as k_base_sample_tiled:
// (sample lo, sample hi, feature group, stream)), log q0 and log|det J| never touch memory, and after
// the last coupling the diagonal-Gaussian target, ybar = gscale * grad log p(y) and the workgroup's
// partial sum of pscale * elbo_j are computed from the registers (src/objectives/elbo.jl:65-70,93-97).
// FUSED with INVERSE (and STASH): the forward-KL step's inverse chain in the same way (src/objectives/loglikelihood.jl:26-33):
// the tile is read from the caller's ys in the standard d x N layout (xt, read only), every coupling inverse leaves its stash,
// and after the last one the seed gt = gscale * grad log q0(z) (k_target_tiled's arithmetic with mu = 0, var = 1) and the
// workgroup's partial sum of pscale * (log q0(z_j) + ladj_inv_j) come from the registers; z itself is not written (the
// reverse pass reads only the stash and the seed).
struct FusedArgs {
  uint32_t k0, k1, stream;
  const uint32_t *stream_ptr;  // non-null: the Philox stream id is read from device memory (hipGraph replay of the step)
  uint64_t off;           // global index of this shard's first sample
  const float *mu, *var;  // diagonal-Gaussian target (test/flow.jl:43-46)
  float *gt;              // ybar out (tiled), or nullptr
  float gscale;
  double *partial;        // [gridDim.x] out
  double pscale;
  float *stash;           // STASH: [tile][coupling][StashGeo<G>::SIZE] out
  long long *trace;       // NF_KERNEL_TRACE builds: clock stamps for tools/trace_chain.py, else unused
  int tkind;              // k_affine_chain_tgt: NF_TARGET_BANANA / FUNNEL / WARPED / CROSS and the target's two scalars
  float ts0, ts1;
};

// B6 (round 4, the default): the conditioner GEMMs on the bf16 matrix cores with six-term products (nf_mfma.h), 2.67 x
// the fp32 MFMA's rate at fp32 accuracy.  The B6 images are 1.5 x the fp32 ones (49 KB per net at hidden 64), so the LDS
// holds THREE of them and rotates per NET instead of two (s, t) pairs per coupling: image i of the workgroup's sequence
// s(c0), t(c0), s(c1), ... lives in slot i mod 3; the phase of image i starts with a workgroup barrier (image i complete,
// everybody done with image i - 1) and then requests image i + 2 into the slot image i - 1 just left.
// NW: wavefronts (= tiles of a group) per workgroup: 8, or 4 for the k_affine_chain_tgt forms that do not fit 256 registers (launch_chain)
// TGT (the body of k_affine_chain_tgt, FUSED forward only): the epilogue evaluates one of the other four built-in targets
// (fa.tkind, nf_target_epilogue.h) instead of the diagonal Gaussian; everything before it is the same code.
template <class G, bool INVERSE, bool FUSED, bool STASH, bool SLIM, bool B6, int NW, bool TGT>
__device__ __forceinline__ void affine_chain_body(ChainArgs a, float *xt, float *__restrict__ ladj, FusedArgs fa) {
  static_assert(STASH || !SLIM, "SLIM is a stash layout");
  static_assert(!TGT || (FUSED && !INVERSE), "the target switch belongs to the fused ELBO forward");
  static_assert(!FUSED || !INVERSE || STASH, "the fused forward-KL chain leaves the stash of its reverse pass");
  static_assert(G::MB == G::CB, "parity blocks must have equal padded size");
  constexpr bool FKL = FUSED && INVERSE;  // forward-KL mode; FUSED && !INVERSE is the ELBO forward
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int IMG2 = 2 * G::SIZE;  // s and t images of one coupling are adjacent in wimg
  constexpr int NV4 = IMG2 / 4;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  const long ntiles = (a.N + NF_TILE - 1) / NF_TILE;
  const long ngroups = (ntiles + NW - 1) / NW;
  // coupling executed at position s of the chain: forward applies the LAST flat coupling first
  auto coupling_at = [&](int s) { return INVERSE ? s : a.ncoup - 1 - s; };

  using BG = B6Geo<G>;
  constexpr int B6F = BG::BYTES / 4;  // floats per B6 image
  // B6: image i of this workgroup's sequence (position (i mod 2 ncoup) / 2 of the chain, net i & 1) -> LDS slot i mod 3, by
  // LDS-DMA; complete at the next workgroup barrier (s_waitcnt vmcnt(0) of every wave for its own pieces)
  const int my_groups = (long)blockIdx.x < ngroups ? (int)((ngroups - blockIdx.x + gridDim.x - 1) / gridDim.x) : 0;
  const int my_images = my_groups * 2 * a.ncoup;
  int req = 0, req_idx = 0, req_slot = 0;  // images requested so far, the next one's index in the chain and its slot
  auto b6_request_next = [&]() {  // requests are issued strictly in sequence order: no division, three small counters
    if (req >= my_images) return;
    typedef __attribute__((address_space(3))) void lds_void_t;
    const int kk = coupling_at(req_idx >> 1);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<unsigned char *>(a.wimg_b6) + (size_t)(2 * kk + (req_idx & 1)) * BG::BYTES, 0, BG::BYTES, 0x00020000);
    float *dstb = lds + req_slot * B6F;
    constexpr int NP = (BG::BYTES + 1023) / 1024;
    for (int p = wave; p < NP; p += NW)
      if (p * 1024 + lane * 16 < BG::BYTES)  // the last piece is partial: its idle lanes must not write
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t *)(dstb + p * 256), 16, lane * 16, p * 1024, 0, 0);
    ++req;
    req_idx = req_idx + 1 == 2 * a.ncoup ? 0 : req_idx + 1;
    req_slot = req_slot == 2 ? 0 : req_slot + 1;
  };
  int cur_slot = 0;  // B6: slot of the next image to be used
  // prologue: image of the first coupling -> buffer 0
  if constexpr (B6) {
    b6_request_next();
    b6_request_next();
  } else {
    const float4 *src = reinterpret_cast<const float4 *>(a.wimg + (long)coupling_at(0) * IMG2);
    float4 *dst = reinterpret_cast<float4 *>(lds);
    for (int i = tid; i < NV4; i += 64 * NW) dst[i] = src[i];
  }
  // FUSED: target parameters by feature, zero padded: tmu[f], tiv[f] = 1/var[f]; tc0 = d log 2pi + sum log var
  constexpr int TP = 64 * G::CB;  // padded feature count (E and O halves)
  float *tmu = lds + (B6 ? 3 * B6F : 2 * IMG2), *tiv = tmu + TP, *tc0 = tiv + TP;
  double *wsum = reinterpret_cast<double *>(tc0 + 2);  // [NW] per-wave partial sums (8-byte aligned: TP even)
  if (FUSED && !FKL && !TGT) {  // as in rqs_chain_body, in place: as a shared call it changes the fused k_rqs_chain forms
    for (int i = tid; i < TP; i += 64 * NW) {
      tmu[i] = i < a.d ? fa.mu[i] : 0.f;
      tiv[i] = i < a.d ? 1.f / fa.var[i] : 0.f;
    }
    if (tid == 0) {
      float c = 1.8378770664093453f * (float)a.d;
      for (int i = 0; i < a.d; ++i) c += logf(fa.var[i]);
      tc0[0] = c;
    }
  }
  double wg_total = 0.0;
  __syncthreads();

  int buf = 0;
  for (long grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const long tile = grp * NW + wave;
    const bool live = tile < ntiles;          // wave-uniform
    const long tl = live ? tile : 0;
    const long j = tl * NF_TILE + l31;
    const bool valid = live && j < a.N;
    const TileIO io = make_tile_io(xt, tl, a.d, l31, hi);
    f32x16 E[G::CB], O[G::MB];
    float zz = 0.f;  // FUSED: this lane's share of ||x||^2
    if constexpr (FKL) {  // (chain_load_ys and chain_draw_base would be these two arms; as calls they change the fused kernels)
      // ys[j * d + f] through one descriptor per tile that spans exactly the tile's samples: lanes of padding samples read 0 from
      // the hardware, features >= d (which would be the next sample's) are zeroed here -- the values the layout conversion and
      // tile_load give the plain chain.  The whole byte offset is per lane (voffset), so every access is range-checked.
      const long nv = a.N - tl * NF_TILE;
      const __amdgpu_buffer_rsrc_t ysr = __builtin_amdgcn_make_buffer_rsrc(
          xt + tl * NF_TILE * a.d, 0, live ? (int)((nv < NF_TILE ? nv : NF_TILE) * a.d * 4) : 0, 0x00020000);
      const int yv = (l31 * a.d + 8 * hi) * 4;
#pragma unroll
      for (int b = 0; b < G::CB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int f0 = 2 * (b * 32 + (r & 3) + 8 * (r >> 2));  // E[b][r] is feature f0 + 8 hi, O[b][r] the one after it
          const float e = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ysr, yv + 4 * f0, 0, 0));
          const float o = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ysr, yv + 4 * f0 + 4, 0, 0));
          const int f = f0 + 8 * hi;
          E[b][r] = valid && f < a.d ? e : 0.f;
          O[b][r] = valid && f + 1 < a.d ? o : 0.f;
        }
    } else if (!FUSED) {
      chain_load_tile(E, O, io, valid);
    } else {
      // registers (b, 4q..4q+3) of E and O are features base..base+7, base = 64b + 16q + 8hi:
      // Philox groups base/4 (-> E0 O0 E1 O1) and base/4 + 1 (-> E2 O2 E3 O3)
      const uint64_t gj = fa.off + (uint64_t)j;
      const uint32_t pstream = fa.stream_ptr ? __builtin_amdgcn_readfirstlane(*fa.stream_ptr) : fa.stream;
#pragma unroll
      for (int b = 0; b < G::CB; ++b)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int base = 64 * b + 16 * q + 8 * hi;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int g = base / 4 + h;
            U4 c = {(uint32_t)gj, (uint32_t)(gj >> 32), (uint32_t)g, pstream};
            const U4 rr = philox4x32_10(c, fa.k0, fa.k1);
            float z[4];
            box_muller<float>(rr.x, rr.y, z[0], z[1]);
            box_muller<float>(rr.z, rr.w, z[2], z[3]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const bool in = (4 * g + e < a.d) && valid;  // features >= d and padding samples stay 0
              const float v = in ? z[e] : 0.f;
              zz += v * v;
              if (e & 1) O[b][4 * q + 2 * h + (e >> 1)] = v;
              else E[b][4 * q + 2 * h + (e >> 1)] = v;
            }
          }
        }
    }
    float lsum = 0.f;
    // the forms that STORE ladj (not FUSED) fold each coupling's log-determinant over the two half-waves on its own, so that
    // nf_layer_apply of every coupling, chained, adds up to the whole chain's ladj bit for bit; the fused forms (the training
    // steps) keep one running sum and fold once
    auto fold_ls = [&](float v) {
      if constexpr (!FUSED) v += __shfl_xor(v, 32);
      return v;
    };
    const bool more_groups = grp + gridDim.x < ngroups;
#pragma unroll 1
    for (int s = 0; s < a.ncoup; s += 2) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int pos = s + half;
        if constexpr (B6) {
          // The phase barrier must see this wave's pieces of the image DMA complete -- NOT its stash stores: the vector-memory
          // counter is in order, so "at most 60 operations outstanding" implies the DMA is done once 61 operations have been
          // issued behind it, while __syncthreads() (vmcnt(0)) would drain the stores to HBM twice per coupling.  The image that
          // the barrier of phase i waits for was requested behind the barrier of phase i - 2 (or in front of the tile group's
          // first barrier, which drains everything): the stash stores of phases i - 2 and i - 1, one s net and one t net in
          // either order, lie behind it, every wave issues them (an idle wave's go to a descriptor of extent 0), and the pieces
          // of the request of phase i - 1 on top.  StashStores counts them without UV, which only flat coupling ncoup - 1
          // stores: 81 + 69 at hidden 64, 49 + 37 at hidden 32, 53 + 37 in the SLIM layout; hidden 64 also has 61 in each phase
          // alone.  Kernels without a stash wait for everything.
          static_assert(!STASH || StashStores<G, SLIM>::S_NET + StashStores<G, SLIM>::T_NET >= 61,
                        "vmcnt(60) at the phase barrier: fewer than 61 stores behind an image request");
          auto phase_barrier = [&](bool first_of_group = false) {
            if (STASH && !first_of_group) {  // (a tile group's first image may have nothing but the DMA behind it)
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
              __builtin_amdgcn_s_waitcnt(0xC07C);  // vmcnt(60) lgkmcnt(0)
              __builtin_amdgcn_s_barrier();
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            } else
              __syncthreads();
          };
          phase_barrier(s == 0 && half == 0);  // this coupling's s image is complete, every wave is done with the image before it
          b6_request_next();  // the image after next, into the slot just vacated
          const int slot_t = cur_slot == 2 ? 0 : cur_slot + 1;
          const float *img_s = lds + cur_slot * B6F, *img_t = lds + slot_t * B6F;
          auto between = [&]() {
            phase_barrier();  // the t image is complete, every wave is done with the s image
            b6_request_next();
          };
          float ls;
          if (STASH) {
            const StashIO st = make_stash_io(fa.stash, tl * a.ncoup + coupling_at(pos), StashGeo<G, SLIM>::SIZE, live, l31, hi);
#ifdef NF_KERNEL_TRACE  // tools/trace_chain.py (as the fp32 form below; stamp 3 = end of the combine, 4 = the same: the barrier opens the NEXT position)
            long long *tr = (fa.trace && blockIdx.x == 0 && (tid & 255) == 0 && pos < 8) ? fa.trace + 32 + (tid >> 8) * 64 + pos * 4 - 1 : nullptr;
#else
            long long *tr = nullptr;
#endif
            const bool keep_uv = coupling_at(pos) == a.ncoup - 1;
            if (INVERSE ? (half == 1) : (half == 0)) ls = coupling_step_stash<G, INVERSE, SLIM, true, false>(img_s, img_t, O, E, l31, hi, st, keep_uv, tr, between);
            else ls = coupling_step_stash<G, INVERSE, SLIM, true, true>(img_s, img_t, E, O, l31, hi, st, keep_uv, tr, between);
            NF_STAMP(tr, 3);
            NF_STAMP(tr, 4);
          } else {
#ifdef NF_KERNEL_TRACE  // stamps [32 + wave/4 * 64 + position * 5 + 0..4] of the second tile group (the first one's images arrive cold)
            long long *tr = (fa.trace && blockIdx.x == 0 && (tid & 255) == 0 && pos < 8 && grp != (long)blockIdx.x && grp == (long)blockIdx.x + gridDim.x)
                                ? fa.trace + 32 + (tid >> 8) * 48 + pos * 5 : nullptr;
#else
            long long *tr = nullptr;
#endif
            if (INVERSE ? (half == 1) : (half == 0)) ls = coupling_step<G, INVERSE, true, decltype(between), NW == 8>(img_s, img_t, O, E, l31, hi, between, tr);
            else ls = coupling_step<G, INVERSE, true, decltype(between), NW == 8>(img_s, img_t, E, O, l31, hi, between, tr);
            NF_STAMP(tr, 4);
          }
          lsum += fold_ls(ls);
          cur_slot = slot_t == 2 ? 0 : slot_t + 1;
          continue;
        }
        // prefetch the next coupling's images (wraps to the first coupling for the next tile group)
        const bool have_next = pos + 1 < a.ncoup || more_groups;
        const int knext = coupling_at(pos + 1 < a.ncoup ? pos + 1 : 0);
        if (have_next) {
          // LDS-DMA (buffer_load_dwordx4 ... lds) straight into the other image buffer: no staging
          // registers, no ds_write pass; complete at the barrier below (s_waitcnt vmcnt(0))
          typedef __attribute__((address_space(3))) void lds_void_t;
          const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.wimg) + (long)knext * IMG2, 0, IMG2 * 4, 0x00020000);
          float *dstb = lds + (buf ^ 1) * IMG2;
          constexpr int NP = (IMG2 * 4 + 1023) / 1024;
          for (int p = wave; p < NP; p += NW)
            if (p * 1024 + lane * 16 < IMG2 * 4)  // the last piece is partial: its idle lanes must not write
              __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t *)(dstb + p * 256), 16, lane * 16, p * 1024, 0, 0);
        }
        const float *img_s = lds + buf * IMG2;
        const float *img_t = img_s + G::SIZE;
        // forward order: position 0 is the last flat coupling (odd index => mask 2:2:d => x1 = O)
        const bool x1_is_O = (coupling_at(pos) & 1) != 0;  // compile-time per (INVERSE, half) when ncoup is even
        float ls;
        if (STASH) {
          const StashIO st = make_stash_io(fa.stash, tl * a.ncoup + coupling_at(pos), StashGeo<G, SLIM>::SIZE, live, l31, hi);
#ifdef NF_KERNEL_TRACE  // tools/trace_chain.py: block 0, waves 0 and 4 (one SIMD), stamps [32 + wave/4 * 64 + position * 4 + 0..3]
          // (the slots the reverse kernels of the same step leave alone)
          long long *tr = (fa.trace && blockIdx.x == 0 && (tid & 255) == 0 && pos < 8) ? fa.trace + 32 + (tid >> 8) * 64 + pos * 4 - 1 : nullptr;
#else
          long long *tr = nullptr;
#endif
          const bool keep_uv = coupling_at(pos) == a.ncoup - 1;
          if (INVERSE ? (half == 1) : (half == 0)) ls = coupling_step_stash<G, INVERSE, SLIM, false, false>(img_s, img_t, O, E, l31, hi, st, keep_uv, tr);
          else ls = coupling_step_stash<G, INVERSE, SLIM, false, true>(img_s, img_t, E, O, l31, hi, st, keep_uv, tr);
          NF_STAMP(tr, 3);
          lsum += fold_ls(ls);
          __syncthreads();
          NF_STAMP(tr, 4);
          buf ^= 1;
          continue;
        } else if (INVERSE ? (half == 1) : (half == 0)) {
          (void)x1_is_O;
          ls = coupling_step<G, INVERSE>(img_s, img_t, O, E, l31, hi);
        } else {
          ls = coupling_step<G, INVERSE>(img_s, img_t, E, O, l31, hi);
        }
        lsum += fold_ls(ls);
        __syncthreads();
        buf ^= 1;
      }
    }
    if (live) {
      // the fused ELBO forward of a stashed training step is called with xt == nullptr: the reverse pass reads the stash and gt
      // only, so the flow output stays in the registers (the epilogue below) -- as the forward-KL form's z always does
      if (!FKL && (!(FUSED && STASH) || xt != nullptr)) {
#pragma unroll
        for (int b = 0; b < G::CB; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            tile_store(io, tile_soff(b, r, 0), E[b][r]);
            tile_store(io, tile_soff(b, r, 1), O[b][r]);
          }
      }
      if constexpr (FUSED) lsum += __shfl_xor(lsum, 32);
      if (!FUSED) {
        if (hi == 0 && valid) ladj[j] = INVERSE ? -lsum : lsum;
      }
    }
    if constexpr (FKL) {
      // loglik_j = log q0(z_j) + ladj_inv_j (ladj_inv = -lsum, what the plain inverse chain stores);  seed = gscale * g with
      // g = -(z - mu) / var = -z exactly, k_target_tiled's diagonal-Gaussian term at mu = 0, var = 1: the split path's bits.
      // log q0 is -d log(2 pi) / 2 - ||z||^2 / 2, as the fused ELBO forward evaluates it (not k_target_tiled's per-feature sum)
      const TileIO gio = make_tile_io(fa.gt, tl, a.d, l31, hi);
#pragma unroll
      for (int b = 0; b < G::CB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float ze = E[b][r], zo = O[b][r];
          zz += ze * ze + zo * zo;  // features >= d and padding samples are 0
          if (live) {
            tile_store(gio, tile_soff(b, r, 0), valid ? fa.gscale * -ze : 0.f);
            tile_store(gio, tile_soff(b, r, 1), valid ? fa.gscale * -zo : 0.f);
          }
        }
      zz += __shfl_xor(zz, 32);
      double contrib = 0.0;
      if (hi == 0 && valid) {
        const float logq = (float)(-0.5 * 1.8378770664093453 * a.d) - 0.5f * zz;
        contrib = fa.pscale * (double)(logq + -lsum);
      }
#pragma unroll
      for (int sft = 16; sft >= 1; sft >>= 1) contrib += __shfl_xor(contrib, sft);  // lanes 0..31 carry the terms
      if (lane == 0) wsum[wave] = contrib;
      __syncthreads();
      if (tid == 0) {
        double sgrp = 0.0;
        for (int w = 0; w < NW; ++w) sgrp += wsum[w];
        wg_total += sgrp;
      }
      __syncthreads();
    }
    if constexpr (TGT) {
      // elbo_j = log p(y_j) - log q0(x_j) + ladj_j ;  ybar = gscale * grad log p(y), p one of Banana / Funnel / WarpedGauss / Cross
      const TileIO gio = make_tile_io(fa.gt ? fa.gt : xt, tl, a.d, l31, hi);
      nf_tile_isolate<G::CB>(E, O);
      const float logp = nf_tile_target<G::CB, NF_TGT_ALL4>(fa.tkind, E, O, a.d, fa.ts0, fa.ts1, l31, hi, gio, fa.gt && live, valid, fa.gscale);
      zz += __shfl_xor(zz, 32);
      double contrib = 0.0;
      if (hi == 0 && valid) {
        const float logq = (float)(-0.5 * 1.8378770664093453 * a.d) - 0.5f * zz;
        const float e = logp - logq + lsum;
        contrib = fa.pscale * (double)e;
      }
#pragma unroll
      for (int sft = 16; sft >= 1; sft >>= 1) contrib += __shfl_xor(contrib, sft);  // lanes 0..31 carry the terms
      if (lane == 0) wsum[wave] = contrib;
      __syncthreads();
      if (tid == 0) {
        double sgrp = 0.0;
        for (int w = 0; w < NW; ++w) sgrp += wsum[w];
        wg_total += sgrp;
      }
      __syncthreads();
    }
    if (FUSED && !FKL && !TGT) {
      // elbo_j = log p(y_j) - log q0(x_j) + ladj_j ;  ybar = gscale * grad log p(y)
      const TileIO gio = make_tile_io(fa.gt ? fa.gt : xt, tl, a.d, l31, hi);
      float t = 0.f;
#pragma unroll
      for (int b = 0; b < G::CB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int fe = 2 * (b * 32 + nf_row(r, hi));
          const float re = E[b][r] - tmu[fe], ro = O[b][r] - tmu[fe + 1];
          const float ge = re * tiv[fe], go = ro * tiv[fe + 1];
          t += re * ge + ro * go;
          if (fa.gt && live) {
            tile_store(gio, tile_soff(b, r, 0), valid ? -fa.gscale * ge : 0.f);
            tile_store(gio, tile_soff(b, r, 1), valid ? -fa.gscale * go : 0.f);
          }
        }
      t += __shfl_xor(t, 32);
      zz += __shfl_xor(zz, 32);
      double contrib = 0.0;
      if (hi == 0 && valid) {
        const float logq = (float)(-0.5 * 1.8378770664093453 * a.d) - 0.5f * zz;
        const float e = -0.5f * (tc0[0] + t) - logq + lsum;
        contrib = fa.pscale * (double)e;
      }
#pragma unroll
      for (int sft = 16; sft >= 1; sft >>= 1) contrib += __shfl_xor(contrib, sft);  // lanes 0..31 carry the terms
      if (lane == 0) wsum[wave] = contrib;
      __syncthreads();
      if (tid == 0) {
        double sgrp = 0.0;
        for (int w = 0; w < NW; ++w) sgrp += wsum[w];
        wg_total += sgrp;
      }
      __syncthreads();
    }
  }
  if (FUSED && tid == 0) fa.partial[blockIdx.x] = wg_total;
}
template <class G, bool INVERSE, bool FUSED = false, bool STASH = false, bool SLIM = false, bool B6 = false>
__global__ __launch_bounds__(512) void k_affine_chain(ChainArgs a, float *xt, float *__restrict__ ladj, FusedArgs fa) {
  affine_chain_body<G, INVERSE, FUSED, STASH, SLIM, B6, 8, false>(a, xt, ladj, fa);
}
// The fused ELBO forward for the Banana, Funnel, WarpedGauss and Cross targets: k_affine_chain<G, false, true, STASH, SLIM, B6>'s
// draws, chain and stash with the target switch as its epilogue (one instantiation per geometry serves the four kinds).
template <class G, bool STASH, bool SLIM = false, bool B6 = false, int NW = 8>
__global__ __launch_bounds__(64 * NW) void k_affine_chain_tgt(ChainArgs a, float *xt, FusedArgs fa) {
  affine_chain_body<G, false, true, STASH, SLIM, B6, NW, true>(a, xt, nullptr, fa);
}

// ------------------------------------------------------------------------------------
// reverse pass of one coupling with invertible recompute
// ------------------------------------------------------------------------------------
// In:  y    = coupling OUTPUT (d x N),  ybar = dL/dy,  lbar = dL/d(ladj) per sample
// Out: y    <- coupling INPUT x (reconstructed: x1 = (y1 - T) exp(-S), realnvp.jl:107),
//      ybar <- dL/dx,
//      slab[blockIdx.x] <- this workgroup's partial sum of dL/dtheta for this coupling.
//
// Two phases inside one launch, each with ONE net in LDS and its dW^T accumulators in
// registers:
//   phase T: T = t(x2);  u = y1 - T -> y1 slots;  delta3 = ybar1;            x2bar += W1t^T d1
//   phase S: S = s(x2);  x1 = u exp(-S) -> y1 slots; delta3 = (ybar1*u + lbar)(1 - S^2);
//            x1bar = ybar1 exp(S) -> ybar1 slots;                            x2bar += W1s^T d1
template <class G>
struct BwdAcc {
  f32x16 w1[G::MB][G::H1B];
  f32x16 w2[G::H1B][G::H2B];
  f32x16 w3[G::H2B][G::CB];
  float b1[G::H1B], b2[G::H2B], b3[G::CB];
};

// fold one wave's accumulators into the LDS image (layout of the weight image)
template <int IB, int OB>
__device__ __forceinline__ void fold_acc(float *__restrict__ w, float *__restrict__ b, const f32x16 (&a)[IB][OB],
                                         const float (&bs)[OB], bool first, int l31, int hi) {
  constexpr int S = 32 * OB + NF_IMG_PAD;
#pragma unroll
  for (int i = 0; i < IB; ++i)
#pragma unroll
    for (int o = 0; o < OB; ++o)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float *p = w + (i * 32 + nf_row(r, hi)) * S + o * 32 + l31;
        *p = first ? a[i][o][r] : *p + a[i][o][r];
      }
#pragma unroll
  for (int o = 0; o < OB; ++o) {
    const float v = bs[o] + __shfl_xor(bs[o], 32);
    if (hi == 0) {
      float *p = b + o * 32 + l31;
      *p = first ? v : *p + v;
    }
  }
}

template <int S>
__device__ __forceinline__ void unstage_dense(const float *__restrict__ img, int rows_pad, float *__restrict__ out,
                                              int nin, int nout, int tid, int nthreads) {
  for (int idx = tid; idx < rows_pad * S; idx += nthreads) {
    const int i = idx / S, o = idx - i * S;
    if (i < nin && o < nout) out[(long)i * nout + o] = img[idx];
  }
}

// Slope masks of the hidden pre-activations (bit r set <=> NOT z[r] > 0, i.e. the leaky-ReLU slope is
// 0.01, as in the oracle's ifelse(x > 0, x, 0.01x)): all the reverse pass needs of a1/a2 besides their
// LDS copies, so the activations themselves can die early.  leakyrelu keeps the sign and the zero, so
// the mask is taken from the post-activation value.  z = +-0 counts as slope 0.01: a real unit reaches
// +0 with zero weights and bias, or at a fresh flow on a conditioner half of exactly 0 (the zero-padded
// rows also do, with a zero cotangent).  Built by nf_sign_mask16 (nf_mfma.h), one subtraction and one
// v_alignbit per element.  (Note for maintainers: __builtin_bit_cast applied directly to a
// vector-element expression such as v[b][r] reads element 0 under hipcc 7.2 -- copy to a scalar first.)
__device__ __forceinline__ float lrelu_slope(unsigned mask, int r) { return nf_mask_slope(mask, r); }
template <int NB>
__device__ __forceinline__ void apply_lrelu_grad(f32x16 (&d)[NB], const unsigned (&m)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b) nf_lrelu_grad16(d[b], m[b]);
}

// per-wave LDS scratch of the reverse pass, [feature][sample] tiles with row stride NF_TS:
//   x2 | a1 | a2 | delta(current layer)
template <class G>
struct BwdLds {
  static constexpr int DROWS = (G::H1B > G::H2B ? (G::H1B > G::CB ? G::H1B : G::CB) : (G::H2B > G::CB ? G::H2B : G::CB));
  static constexpr int OFF_X = 0;
  static constexpr int OFF_A1 = OFF_X + G::MB * 32 * NF_TS;
  static constexpr int OFF_A2 = OFF_A1 + G::H1B * 32 * NF_TS;
  static constexpr int OFF_D = OFF_A2 + G::H2B * 32 * NF_TS;
  static constexpr int SCRATCH = OFF_D + DROWS * 32 * NF_TS;  // floats per wave
  static constexpr int WAVES = 4;
  static constexpr size_t BYTES = (size_t)(G::SIZE + WAVES * SCRATCH) * sizeof(float);
};

// INVD: reverse pass of the INVERSE coupling (forward-KL training) at its output w: `y` holds w and is
// advanced to coupling(w), `ybar` holds the cotangent of w and leaves that of the inverse's input.
//   w1 = (v1 - t) exp(-s), ladj_inv = -sum s:   v1bar = w1bar exp(-s),  sbar = -(w1bar w1 + lbar),  tbar = -v1bar
// Phase S runs first there (it needs w1bar and w1), then phase T.
template <class G, bool PHASE_S, bool FULL, bool INVD = false>
__device__ __forceinline__ void bwd_tile(const CouplingArgs &a, const float *__restrict__ img, float *__restrict__ sc,
                                         BwdAcc<G> &acc, float *__restrict__ y, float *__restrict__ ybar,
                                         const float *__restrict__ lbar, float lbar_const, long tile, int l31, int hi,
                                         long long *tr) {
  using L = BwdLds<G>;
  NF_STAMP(tr, 0);
  const long j = tile * NF_TILE + l31;
  // FULL: N is a multiple of the tile, so no sample mask is needed (feature bounds are handled by
  // the buffer descriptors either way).
  const bool valid = FULL ? true : j < a.N;
  const int par_c = 1 - a.par_t;
  const TileIO yio = make_tile_io(y, tile, a.d, l31, hi);
  const TileIO gio = make_tile_io(ybar, tile, a.d, l31, hi);
  float *sd = sc + L::OFF_D;

  // Every LDS stash write / activation-derivative scaling / tile store below is a SIDE JOB of the
  // neighbouring GEMM (nf_mfma.h): program order is
  //   L1 [stash x2] -> L2 [stash a1] -> L3 [stash a2] -> element-wise ->
  //   dX3 [stash d3] -> dW3 [d2 *= lrelu'] -> dX2 [stash d2] -> dW2 [d1 *= lrelu'] ->
  //   dX1 [stash d1] -> dW1 [x2bar stores]
  f32x16 d3[G::CB], y1[G::CB], g1[G::CB];
  unsigned m1[G::H1B], m2[G::H2B];
  {
    f32x16 xb[G::MB];
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = tile_load(yio, tile_soff(b, r, par_c));  // features >= d read as 0
        xb[b][r] = valid ? v : 0.f;
      }
    NF_STAMP(tr, 1);
    f32x16 a1[G::H1B];
    dense_fwd<G::MB, G::H1B>(img + G::W1, img + G::B1, xb, a1, l31, hi,
                             [&](int e) { scratch_put<G::MB>(sc + L::OFF_X, xb, e, l31, hi); });
#pragma unroll
    for (int b = 0; b < G::H1B; ++b)
      nf_lrelu16(a1[b]);
    sign_masks<G::H1B>(a1, m1);
    f32x16 a2[G::H2B];
    dense_fwd<G::H1B, G::H2B>(img + G::W2, img + G::B2, a1, a2, l31, hi,
                              [&](int e) { scratch_put<G::H1B>(sc + L::OFF_A1, a1, e, l31, hi); });
#pragma unroll
    for (int b = 0; b < G::H2B; ++b)
      nf_lrelu16(a2[b]);
    sign_masks<G::H2B>(a2, m2);
    // operands of the element-wise stage: issued here, consumed after the last forward layer
#pragma unroll
    for (int b = 0; b < G::CB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        y1[b][r] = tile_load(yio, tile_soff(b, r, a.par_t));
        g1[b][r] = tile_load(gio, tile_soff(b, r, a.par_t));
      }
    dense_fwd<G::H2B, G::CB>(img + G::W3, img + G::B3, a2, d3, l31, hi,
                             [&](int e) { scratch_put<G::H2B>(sc + L::OFF_A2, a2, e, l31, hi); });
  }
  NF_STAMP(tr, 2);

  const float lb = valid ? (lbar ? lbar[FULL ? j : (j < a.N ? j : 0)] : lbar_const) : 0.f;
#pragma unroll
  for (int b = 0; b < G::CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = b * 32 + nf_row(r, hi);
      const bool ok = (p < a.c) && valid;  // rows >= c: the loads returned 0, the stores are dropped
      const float yv = y1[b][r], gv = g1[b][r];
      if (INVD && !PHASE_S) {
        tile_store(yio, tile_soff(b, r, a.par_t), yv + d3[b][r]);  // v1 = w1 exp(s) + t
        d3[b][r] = ok ? -gv : 0.f;                                  // T-bar = -v1bar
      } else if (INVD) {
        const float s = nf_tanh(d3[b][r]);
        const float es = nf_exp(s);
        tile_store(yio, tile_soff(b, r, a.par_t), yv * es);            // w1 exp(s)
        tile_store(gio, tile_soff(b, r, a.par_t), nf_fdiv(gv, es));    // v1bar
        d3[b][r] = ok ? -(gv * yv + lb) * (1.f - s * s) : 0.f;         // S-bar through tanh
      } else if (!PHASE_S) {
        tile_store(yio, tile_soff(b, r, a.par_t), yv - d3[b][r]);  // u = x1 * exp(S)
        d3[b][r] = ok ? gv : 0.f;                                   // T-bar = ybar1
      } else {
        const float s = nf_tanh(d3[b][r]);
        const float es = nf_exp(s);
        tile_store(yio, tile_soff(b, r, a.par_t), nf_fdiv(yv, es));  // x1 = u * exp(-s)
        tile_store(gio, tile_soff(b, r, a.par_t), gv * es);             // x1bar
        d3[b][r] = ok ? (gv * yv + lb) * (1.f - s * s) : 0.f;           // S-bar through tanh
      }
    }
  NF_STAMP(tr, 3);

  // ---- layer 3
  f32x16 d2[G::H2B];
  dense_bwd_x<G::H2B, G::CB>(img + G::W3, d3, d2, l31, hi, [&](int e) { scratch_put<G::CB>(sd, d3, e, l31, hi); });
  NF_STAMP(tr, 4);
  wave_lds_fence();
  dw_accumulate<G::H2B, G::CB>(sc + L::OFF_A2, sd, acc.w3, acc.b3, l31, hi, [&](int e) {
    if (e < G::H2B * 16) d2[e >> 4][e & 15] *= lrelu_slope(m2[e >> 4], e & 15);
  });
  NF_STAMP(tr, 5);
  wave_lds_fence();
  // ---- layer 2
  f32x16 d1[G::H1B];
  dense_bwd_x<G::H1B, G::H2B>(img + G::W2, d2, d1, l31, hi, [&](int e) { scratch_put<G::H2B>(sd, d2, e, l31, hi); });
  NF_STAMP(tr, 6);
  wave_lds_fence();
  dw_accumulate<G::H1B, G::H2B>(sc + L::OFF_A1, sd, acc.w2, acc.b2, l31, hi, [&](int e) {
    if (e < G::H1B * 16) d1[e >> 4][e & 15] *= lrelu_slope(m1[e >> 4], e & 15);
  });
  NF_STAMP(tr, 7);
  wave_lds_fence();
  // ---- layer 1: x2bar accumulates ybar2 + W1t^T d1t (phase T) + W1s^T d1s (phase S)
  f32x16 g2[G::MB], gold[G::MB];
#pragma unroll
  for (int b = 0; b < G::MB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) gold[b][r] = tile_load(gio, tile_soff(b, r, par_c));
  dense_bwd_x<G::MB, G::H1B>(img + G::W1, d1, g2, l31, hi, [&](int e) { scratch_put<G::H1B>(sd, d1, e, l31, hi); });
  NF_STAMP(tr, 8);
  wave_lds_fence();
  dw_accumulate<G::MB, G::H1B>(sc + L::OFF_X, sd, acc.w1, acc.b1, l31, hi, [&](int e) {
    if (e < G::MB * 16) tile_store(gio, tile_soff(e >> 4, e & 15, par_c), gold[e >> 4][e & 15] + g2[e >> 4][e & 15]);
  });
  NF_STAMP(tr, 9);
  wave_lds_fence();
  NF_STAMP(tr, 10);
}

// reverse pass of ONE coupling by this workgroup (both phases, fold, slab write)
template <class G, bool FULL, bool INVD = false>
__device__ __forceinline__ void bwd_coupling(const CouplingArgs &a, float *__restrict__ y, float *__restrict__ ybar,
                                             const float *__restrict__ lbar, float lbar_const,
                                             float *__restrict__ slab, long slab_stride, float *lds) {
  float *img = lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform
  const int l31 = lane & 31, hi = lane >> 5;
  float *sc = lds + G::SIZE + wave * BwdLds<G>::SCRATCH;
  const long ntiles = (a.N + NF_TILE - 1) / NF_TILE;
  long long *tr0 = (a.trace && blockIdx.x == 0 && tid == 0) ? a.trace : nullptr;
  if (tr0) tr0[0] = clock64();

#pragma unroll 1
  for (int phase = 0; phase < 2; ++phase) {
    long long *tr = tr0 ? tr0 + 8 + phase * 40 : nullptr;  // [8 + phase*40 + tileidx*12 + slot]
    const bool is_s = INVD ? phase == 0 : phase == 1;      // forward chain: T then S; inverse chain: S then T
    stage_packed<G::SIZE, 256>(img, is_s ? a.img_s : a.img_t, tid);
    __syncthreads();
    if (tr0) tr0[1 + phase * 3] = clock64();
    BwdAcc<G> acc;
    net_zero_acc(acc.w1, acc.b1);
    net_zero_acc(acc.w2, acc.b2);
    net_zero_acc(acc.w3, acc.b3);
#pragma unroll 1
    for (long tile = (long)blockIdx.x * 4 + wave; tile < ntiles; tile += (long)gridDim.x * 4) {
      if (!is_s)
        bwd_tile<G, false, FULL, INVD>(a, img, sc, acc, y, ybar, lbar, lbar_const, tile, l31, hi, tr);
      else
        bwd_tile<G, true, FULL, INVD>(a, img, sc, acc, y, ybar, lbar, lbar_const, tile, l31, hi, tr);
      if (tr) tr += 12;
    }
    if (tr0) tr0[2 + phase * 3] = clock64();
    __syncthreads();  // every wave is done with the weight image and its scratch
    // Each wave drops its accumulators, in image layout, into its own G::SIZE-float region of the
    // (now free) LDS; then all threads add the four copies and write the workgroup's slab with
    // 16-byte stores.  Slabs keep the padded image layout; k_reduce_image_slabs maps them to theta.
    {
      float *mine = lds + wave * G::SIZE;
      fold_acc(mine + G::W1, mine + G::B1, acc.w1, acc.b1, true, l31, hi);
      fold_acc(mine + G::W2, mine + G::B2, acc.w2, acc.b2, true, l31, hi);
      fold_acc(mine + G::W3, mine + G::B3, acc.w3, acc.b3, true, l31, hi);
    }
    __syncthreads();
    {
      const float4 *c0 = reinterpret_cast<const float4 *>(lds);
      float4 *dst = reinterpret_cast<float4 *>(slab + ((long)blockIdx.x * slab_stride + (is_s ? 0 : 1) * (long)G::SIZE));
      constexpr int NV4 = G::SIZE / 4;
      for (int i = tid; i < NV4; i += 256) {
        const float4 p0 = c0[i], p1 = c0[i + NV4], p2 = c0[i + 2 * NV4], p3 = c0[i + 3 * NV4];
        float4 r;
        r.x = (p0.x + p1.x) + (p2.x + p3.x);
        r.y = (p0.y + p1.y) + (p2.y + p3.y);
        r.z = (p0.z + p1.z) + (p2.z + p3.z);
        r.w = (p0.w + p1.w) + (p2.w + p3.w);
        dst[i] = r;
      }
    }
    __syncthreads();  // image is restaged next phase
    if (tr0) tr0[3 + phase * 3] = clock64();
  }
}

template <class G, bool FULL>
__global__ __launch_bounds__(256, 1) void k_affine_bwd(CouplingArgs a, float *__restrict__ y, float *__restrict__ ybar,
                                                       const float *__restrict__ lbar, float lbar_const,
                                                       float *__restrict__ slab, long slab_stride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  bwd_coupling<G, FULL>(a, y, ybar, lbar, lbar_const, slab, slab_stride, lds);
}

// The whole chain's reverse pass in ONE launch.  A wave's tiles never change hands, and coupling k+1
// only reads what the same wave wrote for coupling k (y <- x, ybar <- xbar), so there is no
// cross-workgroup dependency: each workgroup simply walks the couplings in flat order.  Saves the launch
// gap and the ramp-up / tail of seven launches per step.
struct BwdAllArgs {
  const float *wimg;  // [coupling][s|t][G::SIZE]
  const unsigned char *wimg_b6t;  // [coupling][s|t][B6TGeo<G>::BYTES]: the bf16-triple images of the dX GEMMs (pair kernel, PB6)
  long long *trace;
  int d, ncoup;
  long N;
  int no_xbar;  // pair kernel: the caller does not read ybar after the launch (a training step), so the coupling processed last
                // skips dX1 and its tile stores.  0 wherever the input cotangent is an output (nf_flow_bwd*, the tape pullbacks)
};
template <class G, bool FULL, bool INVD>
__global__ __launch_bounds__(256, 1) void k_affine_bwd_all(BwdAllArgs aa, float *__restrict__ y, float *__restrict__ ybar,
                                                           const float *__restrict__ lbar, float lbar_const,
                                                           float *__restrict__ slab, long slab_stride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
#pragma unroll 1
  for (int step = 0; step < aa.ncoup; ++step) {
    const int k = INVD ? aa.ncoup - 1 - step : step;  // the inverse chain's reverse pass runs in execution order
    CouplingArgs a;
    a.theta = nullptr;
    a.img_s = aa.wimg + (size_t)(2 * k) * G::SIZE;
    a.img_t = a.img_s + G::SIZE;
    a.trace = k == 0 ? aa.trace : nullptr;
    a.d = aa.d;
    a.par_t = k & 1;
    a.c = (k & 1) ? aa.d / 2 : (aa.d + 1) / 2;
    a.m = aa.d - a.c;
    a.N = aa.N;
    bwd_coupling<G, FULL, INVD>(a, y, ybar, lbar, lbar_const, slab + (long)k * 2 * G::SIZE, slab_stride, lds);
    // What coupling k + 1 loads are this same wave's stores of coupling k.  They are ordered by the
    // barrier at the end of bwd_coupling (s_waitcnt vmcnt(0): the stores have reached L2) and the vector
    // L1 is write-through, exactly as between the two phases inside one coupling -- no agent-scope fence:
    // on this part that would write back / invalidate the XCD's L2 (measured: 90 instead of 74 us per coupling).
  }
}

// ------------------------------------------------------------------------------------
// reverse pass of the training step from the forward's stash: no recompute
// ------------------------------------------------------------------------------------
// Same mathematics and phase structure as bwd_tile / k_affine_bwd_all (phase T then phase S per coupling, one net in
// LDS, its dW accumulators in registers), but x2 / a1 / a2 arrive from the stash already in the dW operand layout
// (registers, no LDS transpose), s / u / masks arrive in the C layout, and nothing of the forward is recomputed:
// per tile-phase 256 MFMAs instead of 384, the flow state `y` is neither read nor written (it stays the flow output).
template <int NB>
__device__ __forceinline__ void stash_get_T(const StashIO &st, int base, int voff, float (&at)[NB][16]) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(st.rs, voff, (base + b * 1024) * 4 + q * 16, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned bits = w[e];
        at[b][4 * q + e] = __builtin_bit_cast(float, bits);
      }
    }
}
template <int NB>
__device__ __forceinline__ void stash_get_lane(const StashIO &st, int base, f32x16 (&v)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(st.rs, st.vL, (base + b * 1024) * 4 + q * 16, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const unsigned bits = w[e];
        v[b][4 * q + e] = __builtin_bit_cast(float, bits);
      }
    }
}
// a T-layout array back into the C layout it was stored from: the inverse of stash_put_T's address map, element by element
// (per wave instruction two whole 128-byte rows, features nf_row(r, 0) and nf_row(r, 1) of the block)
template <int NB>
__device__ __forceinline__ void stash_get_T_as_lane(const StashIO &st, int base, f32x16 (&v)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      v[b][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(st.rs, st.vT, (base + (b * 32 + (r & 3) + 8 * (r >> 2)) * 32) * 4, 0));
}

// dW^T accumulation with the activation operand in registers: at[ib][t] = a[feature ib*32 + l31][sample 2t + hi]
// CORDER: k-step t contracts the sample (t & 3) + 8 (t >> 2) + 4 hi instead -- the order in which the MFMA C layout holds
// the rows of a recomputed operand (recompute_a1t); the delta tile is read in the same order, the sum is the same sum.
template <bool CORDER>
__device__ __forceinline__ constexpr int dw_sample(int t) { return CORDER ? (t & 3) + 8 * (t >> 2) : 2 * t; }
template <int IB, int OB, class SJ = NoSideJob, bool CORDER = false>
__device__ __forceinline__ void dw_accumulate_reg(const float (&at)[IB][16], const float *__restrict__ sd,
                                                  f32x16 (&acc)[IB][OB], float (&bsum)[OB], int l31, int hi, SJ sj = SJ()) {
  constexpr int TG = 2, NG = 16 / TG;
  const float *pd = sd + l31 * NF_TS + (CORDER ? 4 * hi : hi);
  float dn[TG][OB], dc[TG][OB];
#pragma unroll
  for (int u = 0; u < TG; ++u)
#pragma unroll
    for (int ob = 0; ob < OB; ++ob) dn[u][ob] = pd[ob * 32 * NF_TS + dw_sample<CORDER>(u)];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int u = 0; u < TG; ++u)
#pragma unroll
      for (int ob = 0; ob < OB; ++ob) dc[u][ob] = dn[u][ob];
    if (g + 1 < NG) {
#pragma unroll
      for (int u = 0; u < TG; ++u)
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) dn[u][ob] = pd[ob * 32 * NF_TS + dw_sample<CORDER>((g + 1) * TG + u)];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < TG; ++u) {
#pragma unroll
      for (int ob = 0; ob < OB; ++ob) bsum[ob] += dc[u][ob];
#pragma unroll
      for (int ib = 0; ib < IB; ++ib)
#pragma unroll
        for (int ob = 0; ob < OB; ++ob) {
          acc[ib][ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(at[ib][g * TG + u], dc[u][ob], acc[ib][ob], 0, 0, 0);
          sj(((g * TG + u) * IB + ib) * OB + ob);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// dW^T accumulation on the bf16 matrix cores (six-term products, nf_mfma.h "B6"): same operands as dw_accumulate_reg -- the
// activation operand in registers, at[ib][t] = a[feature][sample 2t + hi], the delta operand from the LDS tile at the same
// samples -- with the sample <-> k-slot assignment  slot (g, hi, j) <-> sample 2 (8 g + j) + hi : registers 8g .. 8g+7 of `at`
// ARE the lane's eight k-values of group g, and the delta reads are the ones the fp32 form issues.  Both operands are split
// here (8 values -> 3 x 4 registers each); 12 bf16 MFMAs of 32 clocks replace 16 fp32 ones of 64 per (ib, ob) block pair.
// The bias gradient stays the fp32 sum of the deltas.
// The activation operand arrives already split (split_T, done by the consumer while it waits for the producer's delta tile:
// 48 registers per 32-feature block pair instead of 32 fp32 + the splits of the group in flight); one delta block's eight
// values and their split are live at a time, the next unit's delta values are requested behind the current unit's MFMAs.
// Pipeline unit = (sample group g, delta block ob).
template <int IB, int OB, class SJ = NoSideJob>
__device__ __forceinline__ void dw_accumulate_reg_b6(const SplitT<IB> &as, const float *__restrict__ sd, f32x16 (&acc)[IB][OB],
                                                     float (&bsum)[OB], int l31, int hi, SJ sj = SJ()) {
  const float *pd = sd + l31 * NF_TS + hi;
  constexpr int NU = 2 * OB;
  float dn[8], dc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dn[j] = pd[2 * j];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int g = u / OB, ob = u % OB;
#pragma unroll
    for (int j = 0; j < 8; ++j) dc[j] = dn[j];
    if (u + 1 < NU) {
      const int g1 = (u + 1) / OB, ob1 = (u + 1) % OB;
#pragma unroll
      for (int j = 0; j < 8; ++j) dn[j] = pd[ob1 * 32 * NF_TS + 2 * (8 * g1 + j)];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) bsum[ob] += dc[j];
    nf_u32x4 dh, dm, dl;
    nf_split8(dc, dh, dm, dl);
    __builtin_amdgcn_sched_barrier(0);
    // smallest terms first (as dense_fwd_b6): al dh, ah dl, am dm, am dh, ah dm, ah dh -- the IB accumulators interleaved
#pragma unroll
    for (int term = 0; term < 6; ++term)
#pragma unroll
      for (int ib = 0; ib < IB; ++ib) {
        const nf_u32x4 &a = term == 0 ? as.l[ib][g] : (term == 2 || term == 3) ? as.m[ib][g] : as.h[ib][g];
        const nf_u32x4 &d = term == 1 ? dl : (term == 2 || term == 4) ? dm : dh;
        acc[ib][ob] = nf_mfma_bf16(a, d, acc[ib][ob]);
        const int c = (u * 6 + term) * IB + ib;  // running MFMA index: two side-job slots each
        sj(2 * c);
        sj(2 * c + 1);
      }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// a1^T = leakyrelu(W1 x2 + b1) as the dW2 GEMM wants it -- lane <-> hidden unit, register r <-> sample
// (r & 3) + 8 (r >> 2) + 4 hi (dw_accumulate_reg<..., CORDER>) -- from the conditioner input in the MFMA C layout:
// D' = x2^T W1^T, i.e. dense_fwd with the operand roles swapped (A: the input's registers, B: the weight image's rows, lanes
// along a row as in the forward fetch).  Same k order and operand values as the forward's own first layer.
template <class G>
__device__ __forceinline__ void recompute_a1t(const float *__restrict__ img, const f32x16 (&x2c)[G::MB], float (&a1t)[G::H1B][16],
                                              int l31, int hi) {
  constexpr int NG = G::MB * 4, S = G::S1, OB = G::H1B;
  f32x16 z[OB];
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    const float bias = img[G::B1 + ob * 32 + l31];
#pragma unroll
    for (int r = 0; r < 16; ++r) z[ob][r] = bias;
  }
  const float *wl = img + G::W1 + (4 * hi) * S + l31;
  float wn[OB][4], wc[OB][4];
#pragma unroll
  for (int ob = 0; ob < OB; ++ob)
#pragma unroll
    for (int e = 0; e < 4; ++e) wn[ob][e] = wl[e * S + ob * 32];
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int ob = 0; ob < OB; ++ob)
#pragma unroll
      for (int e = 0; e < 4; ++e) wc[ob][e] = wn[ob][e];
    if (g + 1 < NG) {
#pragma unroll
      for (int ob = 0; ob < OB; ++ob)
#pragma unroll
        for (int e = 0; e < 4; ++e) wn[ob][e] = wl[((g + 1) * 8 + e) * S + ob * 32];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int ob = 0; ob < OB; ++ob)
        z[ob] = __builtin_amdgcn_mfma_f32_32x32x2f32(x2c[g / 4][(g % 4) * 4 + e], wc[ob][e], z[ob], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int ob = 0; ob < OB; ++ob) {
    nf_lrelu16(z[ob]);
#pragma unroll
    for (int r = 0; r < 16; ++r) a1t[ob][r] = z[ob][r];
  }
}

template <class G>
struct BwdStashLds {
  static constexpr int DROWS = BwdLds<G>::DROWS;
  static constexpr int SCRATCH = DROWS * 32 * NF_TS;  // one delta tile per wave
  static constexpr int WAVES = 4;
  static constexpr int IMGMAX = B6TGeo<G>::BYTES / 4 > G::SIZE ? B6TGeo<G>::BYTES / 4 : G::SIZE;  // fp32 or B6T image
  static constexpr int FLOATS = (IMGMAX + WAVES * SCRATCH) > WAVES * G::SIZE ? (IMGMAX + WAVES * SCRATCH) : WAVES * G::SIZE;
  static constexpr size_t BYTES = (size_t)FLOATS * sizeof(float);  // the fold at the end of a phase needs 4 images
};

// s and x1 (uv; StashGeo) of a phase-S tile are loaded one tile ahead, into the same registers, while the previous tile runs its last
// two GEMMs: every wave of the chip asks for its tile's operands at the same moment (25 MB at once), and without the
// head start the element-wise stage waits 3.5-6.7 k cycles for them (tools/trace_bwd_stashed.py).
// (Round 4, measured and removed: the tile's two cotangent halves requested the same way in the pair kernel's phase S -- 32
// more registers in the producer, no spills, 339-341 us per launch against 338-342 without, and the inverse-direction kernel
// 1 944 us per chunk against 1 680.)
template <class G>
struct StashFirst {
  f32x16 sv[G::CB], uv[G::CB];
};
template <class G, bool SLIM = false>
__device__ __forceinline__ void stash_issue_first(StashFirst<G> &f, float *stash, int k, int ncoup, long tile, int l31, int hi) {
  using SG = StashGeo<G, SLIM>;
  static_assert(G::MB == G::CB, "a neighbour's XT stands in for UV");
  const StashIO st = make_stash_io(stash, tile * ncoup + k, SG::SIZE, true, l31, hi);
  stash_get_lane<G::CB>(st, SG::SV, f.sv);
  if (k + 1 < ncoup) {  // wave-uniform: x1 (INVD: w1) is the conditioner input of flat coupling k + 1, in that slot's XT
    const StashIO nb = make_stash_io(stash, tile * ncoup + k + 1, SG::SIZE, true, l31, hi);
    stash_get_T_as_lane<G::CB>(nb, SG::XT, f.uv);
  } else {
    stash_get_lane<G::CB>(st, SG::UV, f.uv);
  }
}

// INVD: reverse pass of the INVERSE coupling (forward-KL training; algebra as in bwd_tile): the UV slot holds w1, phase S
// runs first (it needs w1bar and w1 and leaves v1bar = w1bar exp(-s) behind), phase T seeds with -v1bar.
// SB6 (round 4): all six GEMMs of the tile on the bf16 matrix cores (dense_bwd_x_b6 / dw_accumulate_reg_b6); `img` is then
// the net's B6T image.  One wave per SIMD: 512 registers, the split operands fit next to the 128 accumulators here.
template <class G, bool PHASE_S, bool FULL, bool INVD = false, bool SB6 = false>
__device__ __forceinline__ void bwd_tile_stashed(const CouplingArgs &a, const float *__restrict__ img, float *__restrict__ sd,
                                                 BwdAcc<G> &acc, StashFirst<G> &f, float *stash, int k, int ncoup,
                                                 float *__restrict__ ybar, const float *__restrict__ lbar, float lbar_const,
                                                 long tile, long next_tile, int l31, int hi, long long *tr = nullptr) {
  NF_STAMP(tr, 0);
  using SG = StashGeo<G>;
  const long j = tile * NF_TILE + l31;
  const bool valid = FULL ? true : j < a.N;
  const int par_c = 1 - a.par_t;
  const TileIO gio = make_tile_io(ybar, tile, a.d, l31, hi);
  const StashIO st = make_stash_io(stash, tile * ncoup + k, SG::SIZE, true, l31, hi);
  constexpr int nbase = SG::NET0 + (PHASE_S ? 0 : SG::NETSZ);
  const int vT = (l31 * 32 + hi * 16) * 4;  // this lane's feature row and sample parity in a T-layout block

  // loads in the order of first use
  f32x16 g1[G::CB];
#pragma unroll
  for (int b = 0; b < G::CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) g1[b][r] = tile_load(gio, tile_soff(b, r, a.par_t));
  const u32x4 mk = __builtin_amdgcn_raw_buffer_load_b128(st.rs, (hi * 32 + l31) * 16, (nbase + SG::MSK) * 4, 0);
  float a2t[G::H2B][16];
  stash_get_T<G::H2B>(st, nbase + SG::A2, vT, a2t);

  NF_STAMP(tr, 1);
  const float lb = valid ? (lbar ? lbar[FULL ? j : (j < a.N ? j : 0)] : lbar_const) : 0.f;
  f32x16 d3[G::CB];
#pragma unroll
  for (int b = 0; b < G::CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = b * 32 + nf_row(r, hi);
      const bool ok = (p < a.c) && valid;
      const float gv = g1[b][r];
      if (!PHASE_S) {
        d3[b][r] = ok ? (INVD ? -gv : gv) : 0.f;  // T-bar = ybar1 (inverse: -v1bar)
      } else if (INVD) {
        const float s = f.sv[b][r];
        tile_store(gio, tile_soff(b, r, a.par_t), nf_fdiv(gv, nf_exp(s)));  // v1bar
        d3[b][r] = ok ? -(gv * f.uv[b][r] + lb) * (1.f - s * s) : 0.f;     // S-bar through tanh (uv = w1)
      } else {
        const float s = f.sv[b][r], e = nf_exp(s);
        tile_store(gio, tile_soff(b, r, a.par_t), gv * e);  // x1bar
        const float u = f.uv[b][r] * e;                      // uv = x1: the forward's own rounded product
        d3[b][r] = ok ? (gv * u + lb) * (1.f - s * s) : 0.f;  // S-bar through tanh
      }
    }
  const unsigned mk0 = mk[0], mk1 = mk[1], mk2 = mk[2], mk3 = mk[3];
  const unsigned m1[2] = {mk0, mk1}, m2[2] = {mk2, mk3};

  NF_STAMP(tr, 2);
  // ---- layer 3
  f32x16 d2[G::H2B];
  const nf_u32x4 *wt = reinterpret_cast<const nf_u32x4 *>(img);  // SB6: the staged image is the net's B6T image
  if constexpr (SB6) dense_bwd_x_b6<G::H2B, G::CB>(wt + B6TGeo<G>::T3, d3, d2, l31, hi, [&](int e) { scratch_put<G::CB>(sd, d3, e, l31, hi); });
  else dense_bwd_x<G::H2B, G::CB>(img + G::W3, d3, d2, l31, hi, [&](int e) { scratch_put<G::CB>(sd, d3, e, l31, hi); });
  float a1t[G::H1B][16];
  stash_get_T<G::H1B>(st, nbase + SG::A1, vT, a1t);
  NF_STAMP(tr, 3);
  wave_lds_fence();
  auto sj3 = [&](int e) {
    if (e < G::H2B * 16) d2[e >> 4][e & 15] *= lrelu_slope(m2[e >> 4], e & 15);
  };
  if constexpr (SB6) {
    SplitT<G::H2B> a2s;
    split_T<G::H2B>(a2t, a2s);
    dw_accumulate_reg_b6<G::H2B, G::CB>(a2s, sd, acc.w3, acc.b3, l31, hi, sj3);
  } else
    dw_accumulate_reg<G::H2B, G::CB>(a2t, sd, acc.w3, acc.b3, l31, hi, sj3);
  NF_STAMP(tr, 4);
  wave_lds_fence();
  // ---- layer 2
  f32x16 d1[G::H1B];
  if constexpr (SB6) dense_bwd_x_b6<G::H1B, G::H2B>(wt + B6TGeo<G>::T2, d2, d1, l31, hi, [&](int e) { scratch_put<G::H2B>(sd, d2, e, l31, hi); });
  else dense_bwd_x<G::H1B, G::H2B>(img + G::W2, d2, d1, l31, hi, [&](int e) { scratch_put<G::H2B>(sd, d2, e, l31, hi); });
  float x2t[G::MB][16];
  stash_get_T<G::MB>(st, SG::XT, vT, x2t);
  NF_STAMP(tr, 5);
  wave_lds_fence();
  auto sj2 = [&](int e) {
    if (e < G::H1B * 16) d1[e >> 4][e & 15] *= lrelu_slope(m1[e >> 4], e & 15);
  };
  if constexpr (SB6) {
    SplitT<G::H1B> a1s;
    split_T<G::H1B>(a1t, a1s);
    dw_accumulate_reg_b6<G::H1B, G::H2B>(a1s, sd, acc.w2, acc.b2, l31, hi, sj2);
  } else
    dw_accumulate_reg<G::H1B, G::H2B>(a1t, sd, acc.w2, acc.b2, l31, hi, sj2);
  NF_STAMP(tr, 6);
  wave_lds_fence();
  // ---- layer 1: x2bar accumulates ybar2 + W1t^T d1t (phase T) + W1s^T d1s (phase S)
  f32x16 g2[G::MB], gold[G::MB];
#pragma unroll
  for (int b = 0; b < G::MB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) gold[b][r] = tile_load(gio, tile_soff(b, r, par_c));
  if (PHASE_S && next_tile >= 0) stash_issue_first<G>(f, stash, k, ncoup, next_tile, l31, hi);
  if constexpr (SB6) dense_bwd_x_b6<G::MB, G::H1B>(wt + B6TGeo<G>::T1, d1, g2, l31, hi, [&](int e) { scratch_put<G::H1B>(sd, d1, e, l31, hi); });
  else dense_bwd_x<G::MB, G::H1B>(img + G::W1, d1, g2, l31, hi, [&](int e) { scratch_put<G::H1B>(sd, d1, e, l31, hi); });
  NF_STAMP(tr, 7);
  wave_lds_fence();
  auto sj1 = [&](int e) {
    if (e < G::MB * 16) tile_store(gio, tile_soff(e >> 4, e & 15, par_c), gold[e >> 4][e & 15] + g2[e >> 4][e & 15]);
  };
  if constexpr (SB6) {
    SplitT<G::MB> x2s;
    split_T<G::MB>(x2t, x2s);
    dw_accumulate_reg_b6<G::MB, G::H1B>(x2s, sd, acc.w1, acc.b1, l31, hi, sj1);
  } else
    dw_accumulate_reg<G::MB, G::H1B>(x2t, sd, acc.w1, acc.b1, l31, hi, sj1);
  wave_lds_fence();
  NF_STAMP(tr, 8);
}

template <class G, bool FULL, bool INVD = false, bool SB6 = false>
__global__ __launch_bounds__(256, 1) void k_affine_bwd_stashed(BwdAllArgs aa, float *stash, float *__restrict__ ybar,
                                                               const float *__restrict__ lbar, float lbar_const,
                                                               float *__restrict__ slab, long slab_stride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *img = lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hi = lane >> 5;
  constexpr int IMGF = SB6 ? B6TGeo<G>::BYTES / 4 : G::SIZE;  // floats of the staged weight image (fp32, or B6T)
  float *sd = lds + IMGF + wave * BwdStashLds<G>::SCRATCH;
  const long ntiles = (aa.N + NF_TILE - 1) / NF_TILE;
  const long tile0 = (long)blockIdx.x * 4 + wave, tstride = (long)gridDim.x * 4;
  StashFirst<G> f;
  // clock stamps of block 0 / thread 0 for tools/trace_bwd_stashed.py (first coupling processed): [0] start;
  // per phase p: [1+4p] image staged, [2+4p] tiles done, [3+4p] every wave done, [4+4p] folded + slab written;
  // [32 + 24p + 12i + 0..8]: stages of tile i (< 2) of phase p
#ifdef NF_KERNEL_TRACE
  long long *tr0 = (aa.trace && blockIdx.x == 0 && tid == 0) ? aa.trace : nullptr;
  if (tr0) tr0[0] = clock64();
#endif
  if (INVD && tile0 < ntiles) stash_issue_first<G>(f, stash, aa.ncoup - 1, aa.ncoup, tile0, l31, hi);  // S runs first
#pragma unroll 1
  for (int step = 0; step < aa.ncoup; ++step) {
    const int k = INVD ? aa.ncoup - 1 - step : step;  // the inverse chain's reverse pass runs in execution order
    CouplingArgs a;
    a.theta = nullptr;
    a.img_s = aa.wimg + (size_t)(2 * k) * G::SIZE;
    a.img_t = a.img_s + G::SIZE;
    a.trace = nullptr;
    a.d = aa.d;
    a.par_t = k & 1;
    a.c = (k & 1) ? aa.d / 2 : (aa.d + 1) / 2;
    a.m = aa.d - a.c;
    a.N = aa.N;
    float *kslab = slab + (long)k * 2 * G::SIZE;
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
      const bool is_s = INVD ? phase == 0 : phase == 1;
      if constexpr (SB6)
        stage_packed<IMGF, 256>(img, reinterpret_cast<const float *>(aa.wimg_b6t + (size_t)(2 * k + (is_s ? 0 : 1)) * B6TGeo<G>::BYTES), tid);
      else
        stage_packed<G::SIZE, 256>(img, is_s ? a.img_s : a.img_t, tid);
      __syncthreads();
      BwdAcc<G> acc;
      net_zero_acc(acc.w1, acc.b1);
      net_zero_acc(acc.w2, acc.b2);
      net_zero_acc(acc.w3, acc.b3);
      NF_STAMP(step == 0 ? tr0 : nullptr, 1 + phase * 4);
#pragma unroll 1
      for (long tile = tile0; tile < ntiles; tile += tstride) {
        const long nt = tile + tstride < ntiles ? tile + tstride : -1;
#ifdef NF_KERNEL_TRACE
        const long ti = (tile - tile0) / tstride;
        long long *tr = (tr0 && step == 0 && ti < 2) ? tr0 + 32 + phase * 24 + ti * 12 : nullptr;
#else
        long long *tr = nullptr;
#endif
        if (!is_s) bwd_tile_stashed<G, false, FULL, INVD, SB6>(a, img, sd, acc, f, stash, k, aa.ncoup, ybar, lbar, lbar_const, tile, nt, l31, hi, tr);
        else bwd_tile_stashed<G, true, FULL, INVD, SB6>(a, img, sd, acc, f, stash, k, aa.ncoup, ybar, lbar, lbar_const, tile, nt, l31, hi, tr);
      }
      NF_STAMP(step == 0 ? tr0 : nullptr, 2 + phase * 4);
      __syncthreads();  // every wave is done with the weight image and its scratch
      NF_STAMP(step == 0 ? tr0 : nullptr, 3 + phase * 4);
      // s and u of the next phase-S's first tile fly behind the fold, the slab write and the staging of the next image
      if (tile0 < ntiles) {
        if (!INVD && !is_s) stash_issue_first<G>(f, stash, k, aa.ncoup, tile0, l31, hi);
        if (INVD && !is_s && step + 1 < aa.ncoup) stash_issue_first<G>(f, stash, k - 1, aa.ncoup, tile0, l31, hi);
      }
      {
        float *mine = lds + wave * G::SIZE;
        fold_acc(mine + G::W1, mine + G::B1, acc.w1, acc.b1, true, l31, hi);
        fold_acc(mine + G::W2, mine + G::B2, acc.w2, acc.b2, true, l31, hi);
        fold_acc(mine + G::W3, mine + G::B3, acc.w3, acc.b3, true, l31, hi);
      }
      __syncthreads();
      {
        const float4 *c0 = reinterpret_cast<const float4 *>(lds);
        float4 *dst = reinterpret_cast<float4 *>(kslab + ((long)blockIdx.x * slab_stride + (is_s ? 0 : 1) * (long)G::SIZE));
        constexpr int NV4 = G::SIZE / 4;
        for (int i = tid; i < NV4; i += 256) {
          const float4 p0 = c0[i], p1 = c0[i + NV4], p2 = c0[i + 2 * NV4], p3 = c0[i + 3 * NV4];
          float4 r;
          r.x = (p0.x + p1.x) + (p2.x + p3.x);
          r.y = (p0.y + p1.y) + (p2.y + p3.y);
          r.z = (p0.z + p1.z) + (p2.z + p3.z);
          r.w = (p0.w + p1.w) + (p2.w + p3.w);
          dst[i] = r;
        }
      }
      __syncthreads();  // image is restaged next phase; ybar stores of this phase are read by the next (same wave)
      NF_STAMP(step == 0 ? tr0 : nullptr, 4 + phase * 4);
    }
  }
}

// ------------------------------------------------------------------------------------
// reverse pass from the stash, TWO wavefronts per tile (k_affine_bwd_pair)
// ------------------------------------------------------------------------------------
// k_affine_bwd_stashed runs one wavefront per SIMD (its 128 dW accumulator registers plus the delta / operand tiles
// need the whole 512-register file), so nothing fills the matrix pipe while that wave fetches operands, scales deltas
// or waits for its stash loads: 0.55 MFMA-busy (profiles/r3a_pmc_summary.json).  Here a tile is shared by a PRODUCER
// wave, which walks the delta chain (element-wise stage, dX3, dX2, dX1: 128 MFMAs, no accumulators) and leaves every
// delta tile in LDS, and a CONSUMER wave on the same SIMD, which owns the net's dW accumulators and contracts the
// stashed activations with those tiles (dW3, dW2, dW1: 128 MFMAs).  Both fit 256 registers, so the SIMD holds both, and
// the three workgroup barriers per tile line the two up GEMM by GEMM with equal MFMA counts on either side
// (32 | 64 | 32): whatever one wave does besides MFMAs is covered by the other's.
//   producer: d3 -> LDS | B1 | dX3, d2 -> LDS | B2 | dX2, d1 -> LDS | B3 | dX1, x2bar
//   consumer: a2 loads  | B1 | dW3 (d3)       | B2 | dW2 (d2)       | B3 | dW1 (d1)
// One buffer per delta suffices: d3 of the next tile is written after B3, when dW3 has long read it (before B2), etc.
// Whole tiles only (d = 64, N a multiple of 32) and every pair the same number of tiles (barriers inside the tile loop).
// PB6 (round 4): the producer's three dX GEMMs on the bf16 matrix cores (dense_bwd_x_b6); the LDS then holds the net's
// B6T image instead of the fp32 one -- nobody else reads weights in this kernel (the consumer contracts activations with
// deltas), except the SLIM stash's a1 recompute, which therefore keeps the fp32 image.
// DW6 (with PB6): the consumer's dW GEMMs on the bf16 cores as well.  The producer splits every cotangent once (it needs the
// triples for its own dX GEMM), leaves them in LDS (split_to_lds_tr: the consumer's ds_read_b64_tr_b16 transposes them, nf_mfma.h)
// instead of the fp32 tile, and the consumer splits only the stashed activations.  Two triple buffers per pair, used alternately
// (d3 | d2 | d1 | next d3 | ...): a buffer is rewritten two barriers after the GEMM that read it.
// Both roles of the DW6 form run in ANTI-PHASE: the producer's stages are [matrix burst | vector burst], the consumer's
// [vector burst | matrix burst] -- two mixed streams on one SIMD add up, a matrix burst and a vector burst overlap
// (tools/probe/mfma_valu_overlap_probe.hip; the woven forms it replaced: tools/experiments/README.md).
#ifndef NF_TRACE_PAIR
#define NF_TRACE_PAIR 0  // trace builds: which of the workgroup's four pairs tools/trace_bwd_pair.py sees
#endif
template <class G, bool PB6 = false, bool DW6 = false>
struct BwdPairLds {
  static_assert(!DW6 || (PB6 && G::CB <= 2 && G::H1B <= 2 && G::H2B <= 2), "triple buffers hold two blocks");
  static constexpr int D3 = 0, D2 = D3 + G::CB * 32 * NF_TS, D1 = D2 + G::H2B * 32 * NF_TS;
  static constexpr int PAIR = DW6 ? 2 * TR_BUF / 4 : D1 + G::H1B * 32 * NF_TS;
  static constexpr int PAIRS = 4;
  static constexpr int IMG = PB6 ? B6TGeo<G>::BYTES / 4 : G::SIZE;  // floats of the staged weight image
  static constexpr int FLOATS = (IMG + PAIRS * PAIR) > PAIRS * G::SIZE ? (IMG + PAIRS * PAIR) : PAIRS * G::SIZE;
  static constexpr size_t BYTES = (size_t)FLOATS * sizeof(float);  // the fold at the end of a phase needs 4 images
};

// Cotangent residency (forward direction; the inverse direction, whose phase S runs first, parks nothing).  A pair owns the same
// tiles in both phases of a coupling, and between the two the tile's cotangent used to make a round trip through memory: phase T
// loaded both halves and stored conditioner half + g2t, phase S loaded both again.  For the first NF_PAIR_PARK tiles of a pair the
// producer keeps them instead: phase T parks g2t (W1^T d1 of the t net) and, for the first NF_PAIR_PARK_G1 tiles, the transformed
// half's cotangent, and does not touch the conditioner half at all; phase S builds d3 from the parked registers, asks for the
// conditioner half behind B3, where only the closing stores need it, and stores (half + g2t) + g2s -- the two additions in the
// order the round trip gave them, so the bits do not change.  The producer has the registers: the kernel is allocated 256 per wave
// for the consumer's sake.  Tiles beyond the parked ones (more than two rounds) keep the round trip, in the body they always had.
// 2 x 16 + 1 x 16 parked registers: with the second tile's g1 as well the unparked body (64 parked + its own early conditioner
// half) no longer fits -- 56 / 80 bytes of scratch in the whole-batch / ragged forms (tests/test_cotangent_residency_cpu.py).
// Carry across the coupling boundary (forward direction).  The masks alternate and a pair's tiles never change hands, so the
// conditioner half's outgoing cotangent (half + g2t) + g2s that phase S of coupling k stores is the transformed half's cotangent g1
// that the same wave loads at the head of phase T of coupling k + 1.  For the parked tiles it stays in registers instead: slot 0's
// goes straight into g1[0] of the next coupling (and is not stored while another coupling follows in the launch: its phase S
// takes g1 from there as well); slot 1's into `cy`, which dies at the head of the next phase T's slot-1 body, before g2[1] is
// born (its phase S still re-reads the half from memory, so its store stays) -- the live peak stays 48 registers.  The first
// processed coupling's g1 of both tiles is loaded into the same registers in front of the coupling loop, so that no body has a
// run-time branch around its prologue loads.  The same bits either way: the value kept is the value stored.
// Both parked slots carry, in whole batches at d = 64 (FULL) only: in the ragged / d < 64 form the masks' state no longer fits beside a carried tile, which
// phase S's slot-1 body holds on top of its own parked registers -- 20 bytes of scratch with both slots carried, 12 with slot 0
// alone.  That form keeps the round trip between couplings.
#define NF_PAIR_PARK 2
#define NF_PAIR_PARK_G1 1
template <class G>
struct PairPark {
  f32x16 g1[NF_PAIR_PARK_G1][G::CB], g2[NF_PAIR_PARK][G::MB];
  f32x16 cy[G::CB];  // slot 1's carry
};

// FULL: d = 64 and N a multiple of the tile (no sample / feature masks).  INVD: reverse pass of the INVERSE coupling
// (forward-KL training; algebra of bwd_tile_stashed: phase S first, the UV slot holds w1).  live: this pair has a tile in
// this round of the workgroup's tile loop -- a pair without one only keeps the barrier count.
// SLOT: the tile's parked registers (< 0: none, the cotangent goes through memory as it always did -- the body is then the one
// this kernel had before parking; the inverse direction has no other).  A template parameter, so that every body knows which
// parked registers are live around it.  last: nobody reads this coupling's input cotangent (BwdAllArgs::no_xbar, coupling
// processed last): no dX1 and no tile stores -- the closing ones behind one wave-uniform branch, phase S's x1bar through a
// descriptor of extent 0, which the hardware drops, so that the tile's prologue stays free of branches.  more: another coupling
// follows in this launch (a carried slot 0 then keeps its closing value and does not store it).
template <class G, bool PHASE_S, bool FULL, bool INVD, bool SLIM, bool PB6, bool DW6, int SLOT>
__device__ __forceinline__ void pair_produce(const CouplingArgs &a, const float *__restrict__ img, float *__restrict__ sp,
                                             StashFirst<G> &f, PairPark<G> &pk, bool last, bool more, float *stash, int k, int ncoup,
                                             float *__restrict__ ybar, const float *__restrict__ lbar, float lbar_const, long tile,
                                             long next_tile, bool live, int l31, int hi, int par, long long *tr = nullptr) {
  using SG = StashGeo<G, SLIM>;
  using L = BwdPairLds<G, PB6, DW6>;
  char *bufa = reinterpret_cast<char *>(sp) + par * TR_BUF, *bufb = reinterpret_cast<char *>(sp) + (par ^ 1) * TR_BUF;  // DW6
  if (!live) {
    __syncthreads();
    __syncthreads();
    __syncthreads();
    return;
  }
  NF_STAMP(tr, 0);
  const long j = tile * NF_TILE + l31;
  const bool valid = FULL ? true : j < a.N;
  const int par_c = 1 - a.par_t;
  const TileIO gio = make_tile_io(ybar, tile, a.d, l31, hi);
  const StashIO st = make_stash_io(stash, tile * ncoup + k, SG::SIZE, true, l31, hi);
  constexpr int nbase = SG::NET0 + (PHASE_S ? 0 : SG::NETSZ);
  static_assert(!INVD || SLOT < 0, "the inverse direction parks nothing");
  constexpr bool FIRST = PHASE_S == INVD;  // the coupling's first phase
  constexpr bool parked = SLOT >= 0, parked1 = SLOT >= 0 && SLOT < NF_PAIR_PARK_G1;
  constexpr int S2 = SLOT < 0 ? 0 : SLOT, S1 = parked1 ? SLOT : 0;
  constexpr bool carried = !INVD && SLOT >= 0 && SLOT < (FULL ? 2 : 0);  // g1 of phase T arrives in registers, phase S leaves the next one
  static_assert(!carried || (G::CB == G::MB && SLOT < 2), "a conditioner half becomes a transformed half");
  f32x16 g1[G::CB];
  if constexpr (carried && !PHASE_S) {
#pragma unroll
    for (int b = 0; b < G::CB; ++b) g1[b] = SLOT == 0 ? pk.g1[0][b] : pk.cy[b];
  } else if constexpr (FIRST || !parked1) {
#pragma unroll
    for (int b = 0; b < G::CB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) g1[b][r] = tile_load(gio, tile_soff(b, r, a.par_t));
  } else {
#pragma unroll
    for (int b = 0; b < G::CB; ++b) g1[b] = pk.g1[S1][b];
  }
  const u32x4 mk = __builtin_amdgcn_raw_buffer_load_b128(st.rs, (hi * 32 + l31) * 16, (nbase + SG::MSK) * 4, 0);
  f32x16 gold[G::MB];
  if constexpr (!parked) {
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) gold[b][r] = tile_load(gio, tile_soff(b, r, par_c));
  }
  TileIO gx = gio;  // phase S (forward direction): where x1bar goes -- nowhere for the last coupling of a training step
  if constexpr (PHASE_S && !INVD)
    gx.rs = __builtin_amdgcn_make_buffer_rsrc(ybar + tile * a.d * NF_TILE, 0, last ? 0 : a.d * NF_TILE * 4, 0x00020000);
  const float lb = valid ? (lbar ? lbar[FULL ? j : (j < a.N ? j : 0)] : lbar_const) : 0.f;
  f32x16 d3[G::CB];
#pragma unroll
  for (int b = 0; b < G::CB; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const bool ok = (b * 32 + nf_row(r, hi) < a.c) && valid;
      const float gv = g1[b][r];
      if (!PHASE_S) {
        d3[b][r] = ok ? (INVD ? -gv : gv) : 0.f;  // T-bar = ybar1 (inverse: -v1bar)
      } else if (INVD) {
        const float sv = f.sv[b][r];
        tile_store(gio, tile_soff(b, r, a.par_t), nf_fdiv(gv, nf_exp(sv)));  // v1bar (phase T's seed: stored by the last coupling, too)
        d3[b][r] = ok ? -(gv * f.uv[b][r] + lb) * (1.f - sv * sv) : 0.f;    // S-bar through tanh (uv = w1)
      } else {
        const float sv = f.sv[b][r], e = nf_exp(sv);
        tile_store(gx, tile_soff(b, r, a.par_t), gv * e);         // x1bar
        const float u = f.uv[b][r] * e;                           // uv = x1: the forward's own rounded product
        d3[b][r] = ok ? (gv * u + lb) * (1.f - sv * sv) : 0.f;  // S-bar through tanh
      }
    }
  if constexpr (FIRST && parked1 && !carried) {  // the bits the second phase would load: phase T never writes these slots
#pragma unroll
    for (int b = 0; b < G::CB; ++b) pk.g1[S1][b] = g1[b];
  }
  SplitC<DW6 ? G::CB : 1> s3;
  if constexpr (DW6) {
    split_C<G::CB>(d3, s3);
    split_to_lds_tr<G::CB>(bufa, s3, l31, hi);
  } else {
    tile_to_scratch<G::CB>(sp + L::D3, d3, l31, hi);
  }
  unsigned m1[G::H1B], m2[G::H2B];
#pragma unroll
  for (int b = 0; b < G::H1B; ++b) m1[b] = mk[b];
#pragma unroll
  for (int b = 0; b < G::H2B; ++b) m2[b] = mk[2 + b];
  NF_STAMP(tr, 1);
  __syncthreads();  // B1: d3 is in LDS (and the consumer is done with the previous tile's d1)
  NF_STAMP(tr, 2);
  f32x16 d2[G::H2B];
  const nf_u32x4 *wt = reinterpret_cast<const nf_u32x4 *>(img);  // PB6: the staged image is the net's B6T image
  SplitC<DW6 ? G::H2B : 1> s2;
  // DW6: the lane's two chunk addresses in the pair's first hand-over buffer (split_to_lds_tr's)
  const int xw = (l31 >> 2) & 3;
  char *const pw0 = reinterpret_cast<char *>(sp) + l31 * 32 + 8 * (hi ^ xw), *const pw1 = reinterpret_cast<char *>(sp) + l31 * 32 + 8 * ((2 + hi) ^ xw);
  if constexpr (DW6) {  // the GEMM as ONE burst of matrix instructions, then ONE burst of vector work: slopes, split, hand-over stores
    const PairPost<G::H2B> post{d2, m2, s2, pw0 + (bufb - reinterpret_cast<char *>(sp)), pw1 + (bufb - reinterpret_cast<char *>(sp))};
    dense_bwd_x_b6s<G::H2B, G::CB>(wt + B6TGeo<G>::T3, s3, d2, l31, hi);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int b = 0; b < G::H2B; ++b) post.all(b);
  } else {
    if constexpr (PB6) dense_bwd_x_b6<G::H2B, G::CB>(wt + B6TGeo<G>::T3, d3, d2, l31, hi);
    else dense_bwd_x<G::H2B, G::CB>(img + G::W3, d3, d2, l31, hi);
    apply_lrelu_grad<G::H2B>(d2, m2);
    tile_to_scratch<G::H2B>(sp + L::D2, d2, l31, hi);
  }
  NF_STAMP(tr, 3);
  __syncthreads();  // B2
  NF_STAMP(tr, 4);
  f32x16 d1[G::H1B];
  SplitC<DW6 ? G::H1B : 1> s1;
  if constexpr (DW6) {
    const PairPost<G::H1B> post{d1, m1, s1, pw0 + (bufa - reinterpret_cast<char *>(sp)), pw1 + (bufa - reinterpret_cast<char *>(sp))};
    dense_bwd_x_b6s<G::H1B, G::H2B>(wt + B6TGeo<G>::T2, s2, d1, l31, hi);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int b = 0; b < G::H1B; ++b) post.all(b);
  } else {
    if constexpr (PB6) dense_bwd_x_b6<G::H1B, G::H2B>(wt + B6TGeo<G>::T2, d2, d1, l31, hi);
    else dense_bwd_x<G::H1B, G::H2B>(img + G::W2, d2, d1, l31, hi);
    apply_lrelu_grad<G::H1B>(d1, m1);
    tile_to_scratch<G::H1B>(sp + L::D1, d1, l31, hi);
  }
  NF_STAMP(tr, 5);
  __syncthreads();  // B3
  NF_STAMP(tr, 6);
  if (PHASE_S && next_tile >= 0) stash_issue_first<G, SLIM>(f, stash, k, ncoup, next_tile, l31, hi);
  if (last) {  // the input cotangent of the whole flow: not read by the training step that set no_xbar
    NF_STAMP(tr, 7);
    return;
  }
  if constexpr (!FIRST && parked) {  // the conditioner half's cotangent, needed by the closing stores only: in flight behind the GEMM
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) gold[b][r] = tile_load(gio, tile_soff(b, r, par_c));
  }
  f32x16 g2[G::MB];
  if constexpr (DW6) dense_bwd_x_b6s<G::MB, G::H1B>(wt + B6TGeo<G>::T1, s1, g2, l31, hi);
  else if constexpr (PB6) dense_bwd_x_b6<G::MB, G::H1B>(wt + B6TGeo<G>::T1, d1, g2, l31, hi);
  else dense_bwd_x<G::MB, G::H1B>(img + G::W1, d1, g2, l31, hi);
  if constexpr (!parked) {
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) tile_store(gio, tile_soff(b, r, par_c), gold[b][r] + g2[b][r]);
  } else if constexpr (FIRST) {
#pragma unroll
    for (int b = 0; b < G::MB; ++b) pk.g2[S2][b] = g2[b];
  } else if constexpr (carried) {  // the next coupling's g1: kept, and stored where somebody reads it from memory
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float nv = (gold[b][r] + pk.g2[S2][b][r]) + g2[b][r];
        if constexpr (SLOT == 0) pk.g1[0][b][r] = nv;
        else pk.cy[b][r] = nv;
      }
    if (SLOT != 0 || !more) {  // slot 0: only the coupling processed last (the pullback's input cotangent)
#pragma unroll
      for (int b = 0; b < G::MB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) tile_store(gio, tile_soff(b, r, par_c), SLOT == 0 ? pk.g1[0][b][r] : pk.cy[b][r]);
    }
  } else {
#pragma unroll
    for (int b = 0; b < G::MB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) tile_store(gio, tile_soff(b, r, par_c), (gold[b][r] + pk.g2[S2][b][r]) + g2[b][r]);
  }
  NF_STAMP(tr, 7);
}

// (Round 6, measured and removed: the consumer held back by s_sleep behind each barrier -- 256 / 512 / 768 clocks in stage 1,
// twice that in stage 2 -- so that its matrix instructions would run beside the producer's vector tail instead of beside its
// GEMM: 323.2-325.2 against 325.5 us on one box, nothing.  The older wave already wins the arbitration.)
// (Measured and removed: dW1 of a tile moved in front of the NEXT tile's first barrier, where the producer issues no
// MFMAs -- 374-379 us against 366 in one process; and the producer's next-unit operands requested behind B3 -- 370.)
// (Measured and removed: the NEXT tile's a2 requested behind B3 -- 32 more registers across the loop's back edge, which
// hipcc spills to scratch right behind the loads: 428 us per launch against 345.)
template <class G, bool SLIM, bool PB6 = false, bool DW6 = false>
// (`sp` is NOT __restrict__: the DW6 triple buffers are rewritten by the producer between this wave's GEMMs, and through a
// const restrict pointer hipcc reuses the registers of an earlier read of the same address across the barriers.)
__device__ __forceinline__ void pair_consume(const float *__restrict__ img, const float *sp, BwdAcc<G> &acc, float *stash,
                                             int k, int ncoup, long tile, bool is_s, bool live, int l31, int hi, int par,
                                             long long *tr = nullptr) {
  using SG = StashGeo<G, SLIM>;
  using L = BwdPairLds<G, PB6, DW6>;
  if (!live) {
    __syncthreads();
    __syncthreads();
    __syncthreads();
    return;
  }
  NF_STAMP(tr, 0);
  const int nbase = SG::NET0 + (is_s ? 0 : SG::NETSZ);
  const StashIO st = make_stash_io(stash, tile * ncoup + k, SG::SIZE, true, l31, hi);
  const int vT = (l31 * 32 + hi * 16) * 4;
  if constexpr (DW6) {
    const char *bufa = reinterpret_cast<const char *>(sp) + par * TR_BUF, *bufb = reinterpret_cast<const char *>(sp) + (par ^ 1) * TR_BUF;
    // ANTI-PHASE (round 6): two MIXED matrix + vector streams on one SIMD add up, a matrix burst and a vector burst overlap
    // (tools/probe/mfma_valu_overlap_probe.hip).  So every stage of this wave is [split the stage's own activation operand | dW GEMM],
    // the producer's [dX GEMM | slopes, split, hand-over stores]: while one wave is in its matrix burst the other is in its vector
    // burst.  The operand of stage k + 1 is requested at the head of stage k, in front of stage k's split; only one operand's
    // triples are live at a time.
    float a1t[G::H1B][16], x2t[G::MB][16];
    {
      float a2t[G::H2B][16];
      stash_get_T<G::H2B>(st, nbase + SG::A2, vT, a2t);
      NF_STAMP(tr, 1);
      __syncthreads();  // B1
      NF_STAMP(tr, 2);
      SplitT<G::H2B> a2s;
      stash_get_T<G::H1B>(st, nbase + SG::A1, vT, a1t);
      split_T<G::H2B>(a2t, a2s);
      __builtin_amdgcn_sched_barrier(0);
      dw_accumulate_tr6<G::H2B, G::CB>(a2s, bufa, acc.w3, acc.b3, l31, hi);
    }
    NF_STAMP(tr, 3);
    __syncthreads();  // B2
    NF_STAMP(tr, 4);
    {
      SplitT<G::H1B> a1s;
      stash_get_T<G::MB>(st, SG::XT, vT, x2t);
      split_T<G::H1B>(a1t, a1s);
      __builtin_amdgcn_sched_barrier(0);
      dw_accumulate_tr6<G::H1B, G::H2B>(a1s, bufb, acc.w2, acc.b2, l31, hi);
    }
    NF_STAMP(tr, 5);
    __syncthreads();  // B3
    NF_STAMP(tr, 6);
    {
      SplitT<G::MB> x2s;
      split_T<G::MB>(x2t, x2s);
      __builtin_amdgcn_sched_barrier(0);
      dw_accumulate_tr6<G::MB, G::H1B>(x2s, bufa, acc.w1, acc.b1, l31, hi);
    }
    NF_STAMP(tr, 7);
    return;  // (the dW1 block below belongs to the two fp32-tile forms)
  } else if constexpr (SLIM) {
    // a1 is not in the stash: rebuilt here, in this wave's MFMA-free prologue (the producer is in its own: operand loads,
    // element-wise stage, d3 -> LDS), from x2 in the C layout and the W1 rows of the staged image
    float a1t[G::H1B][16];
    {
      f32x16 x2c[G::MB];
      stash_get_lane<G::MB>(st, SG::XL, x2c);
      float a2t[G::H2B][16];
      stash_get_T<G::H2B>(st, nbase + SG::A2, vT, a2t);
      recompute_a1t<G>(img, x2c, a1t, l31, hi);
      NF_STAMP(tr, 1);
      __syncthreads();  // B1
      NF_STAMP(tr, 2);
      dw_accumulate_reg<G::H2B, G::CB>(a2t, sp + L::D3, acc.w3, acc.b3, l31, hi);
    }
    NF_STAMP(tr, 3);
    __syncthreads();  // B2
    NF_STAMP(tr, 4);
    dw_accumulate_reg<G::H1B, G::H2B, NoSideJob, true>(a1t, sp + L::D2, acc.w2, acc.b2, l31, hi);
  } else {
    {
      float a2t[G::H2B][16];
      stash_get_T<G::H2B>(st, nbase + SG::A2, vT, a2t);
      NF_STAMP(tr, 1);
      __syncthreads();  // B1
      NF_STAMP(tr, 2);
      dw_accumulate_reg<G::H2B, G::CB>(a2t, sp + L::D3, acc.w3, acc.b3, l31, hi);
    }
    {
      float a1t[G::H1B][16];
      stash_get_T<G::H1B>(st, nbase + SG::A1, vT, a1t);
      NF_STAMP(tr, 3);
      __syncthreads();  // B2
      NF_STAMP(tr, 4);
      dw_accumulate_reg<G::H1B, G::H2B>(a1t, sp + L::D2, acc.w2, acc.b2, l31, hi);
    }
  }
  {
    float x2t[G::MB][16];
    stash_get_T<G::MB>(st, SG::XT, vT, x2t);
    NF_STAMP(tr, 5);
    __syncthreads();  // B3
    NF_STAMP(tr, 6);
    dw_accumulate_reg<G::MB, G::H1B>(x2t, sp + L::D1, acc.w1, acc.b1, l31, hi);
    NF_STAMP(tr, 7);
  }
}

// the two roles' common step of a phase: the slab write after the consumers' fold
template <class G>
__device__ __forceinline__ void pair_slab_write(const float *__restrict__ lds, float *__restrict__ dstf, int tid) {
  const float4 *c0 = reinterpret_cast<const float4 *>(lds);
  constexpr int NV4 = G::SIZE / 4;
  // through a buffer descriptor: the slab's base is wave-uniform and the element offset 32 bits wide -- as a flat pointer the
  // 64-bit per-lane address of this loop cost the consumer two registers it does not have (12 bytes of scratch, round 5)
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(dstf, 0, G::SIZE * 4, 0x00020000);
  for (int i = tid; i < NV4; i += 512) {
    const float4 p0 = c0[i], p1 = c0[i + NV4], p2 = c0[i + 2 * NV4], p3 = c0[i + 3 * NV4];
    u32x4 r;
    r[0] = __builtin_bit_cast(unsigned, (p0.x + p1.x) + (p2.x + p3.x));
    r[1] = __builtin_bit_cast(unsigned, (p0.y + p1.y) + (p2.y + p3.y));
    r[2] = __builtin_bit_cast(unsigned, (p0.z + p1.z) + (p2.z + p3.z));
    r[3] = __builtin_bit_cast(unsigned, (p0.w + p1.w) + (p2.w + p3.w));
    nf_buffer_store_b128(r, rs, i * 16, 0);
  }
}

// The role branch is the OUTERMOST statement: the producer's prefetch registers and the consumer's accumulators then
// never count against the other role's 256 registers (inside the coupling loop both are live across either branch).
// Every wave executes the same barriers: per phase 1 (image staged) + 3 per round of the tile loop + 3 (tiles done,
// folded, slab written); the tile loop runs as many rounds as the workgroup's first pair needs.
template <class G, bool FULL, bool INVD, bool SLIM, bool PB6 = false, bool DW6 = false>
__global__ __launch_bounds__(512) void k_affine_bwd_pair(BwdAllArgs aa, float *stash, float *__restrict__ ybar,
                                                         const float *__restrict__ lbar, float lbar_const,
                                                         float *__restrict__ slab, long slab_stride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float *img = lds;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pair = wave & 3, role = wave >> 2;  // waves p and p + 4 sit on the same SIMD; role 0 produces, 1 consumes
  const int l31 = lane & 31, hi = lane >> 5;
  static_assert(!(SLIM && PB6), "the SLIM stash's a1 recompute reads the fp32 image");
  using PL = BwdPairLds<G, PB6, DW6>;
  using BT = B6TGeo<G>;
  float *sp = lds + PL::IMG + pair * PL::PAIR;
  auto stage_image = [&](int k, bool is_s) {  // the net's weight image of this phase -> LDS (fp32, or B6T for the producer's dX GEMMs)
    if constexpr (PB6)
      stage_packed<BT::BYTES / 4, 512>(img, reinterpret_cast<const float *>(aa.wimg_b6t + (size_t)(2 * k + (is_s ? 0 : 1)) * BT::BYTES), tid);
    else
      stage_packed<G::SIZE, 512>(img, aa.wimg + (size_t)(2 * k + (is_s ? 0 : 1)) * G::SIZE, tid);
  };
  const long ntiles = (aa.N + NF_TILE - 1) / NF_TILE;
  const long tile0 = (long)blockIdx.x * 4 + pair, tstride = (long)gridDim.x * 4;
  const long wg0 = (long)blockIdx.x * 4;
  const int rounds = wg0 < ntiles ? (int)((ntiles - wg0 + tstride - 1) / tstride) : 0;
  if (role == 0) {
    StashFirst<G> f;
    if (INVD && tile0 < ntiles) stash_issue_first<G, SLIM>(f, stash, aa.ncoup - 1, aa.ncoup, tile0, l31, hi);  // S runs first
    PairPark<G> pk;  // g1 / g2: written in the coupling's first phase, read in its second; g1[0] / cy: carried to the next coupling
    if constexpr (!INVD && FULL) {  // the first coupling's g1 of the carried tiles (coupling 0 transforms the even half)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const long tile = tile0 + s * tstride;
        if (tile < ntiles) {
          const TileIO gio = make_tile_io(ybar, tile, aa.d, l31, hi);
#pragma unroll
          for (int b = 0; b < G::CB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              const float v = tile_load(gio, tile_soff(b, r, 0));
              if (s == 0) pk.g1[0][b][r] = v;
              else pk.cy[b][r] = v;
            }
        }
      }
    }
#pragma unroll 1
    for (int step = 0; step < aa.ncoup; ++step) {
      const int k = INVD ? aa.ncoup - 1 - step : step;  // the inverse chain's reverse pass runs in execution order
      const bool last = aa.no_xbar != 0 && step + 1 == aa.ncoup, more = step + 1 < aa.ncoup;
      CouplingArgs a;
      a.theta = nullptr;
      a.img_s = aa.wimg + (size_t)(2 * k) * G::SIZE;
      a.img_t = a.img_s + G::SIZE;
      a.trace = nullptr;
      a.d = aa.d;
      a.par_t = k & 1;
      a.c = (k & 1) ? aa.d / 2 : (aa.d + 1) / 2;
      a.m = aa.d - a.c;
      a.N = aa.N;
#pragma unroll 1
      for (int phase = 0; phase < 2; ++phase) {
        const bool is_s = INVD ? phase == 0 : phase == 1;
#ifdef NF_KERNEL_TRACE  // the phase boundary: producer stamps [32 + phase 8 + 0..7], consumer [96 + ...]
        long long *trb = (aa.trace && blockIdx.x == 0 && tid == 64 * NF_TRACE_PAIR && step == 0) ? aa.trace + 32 + phase * 8 : nullptr;
#endif
        NF_STAMP(trb, 0);
        stage_image(k, is_s);
        NF_STAMP(trb, 1);
        __syncthreads();
        NF_STAMP(trb, 2);
        auto produce = [&](int it, auto slot) {
          constexpr int SLOT = decltype(slot)::value;
          const long tile = tile0 + (long)it * tstride;
          const long nt = tile + tstride < ntiles ? tile + tstride : -1;
#ifdef NF_KERNEL_TRACE  // tools/trace_bwd_pair.py: block 0, pair 0, first coupling; producer stamps [phase 16 + tile 8 + 0..7]
          long long *tr = (aa.trace && blockIdx.x == 0 && tid == 64 * NF_TRACE_PAIR && step == 0 && it < 2) ? aa.trace + phase * 16 + it * 8 : nullptr;
#else
          long long *tr = nullptr;
#endif
          if (!is_s) pair_produce<G, false, FULL, INVD, SLIM, PB6, DW6, SLOT>(a, img, sp, f, pk, last, more, stash, k, aa.ncoup, ybar, lbar, lbar_const, tile, nt, tile < ntiles, l31, hi, it & 1, tr);
          else pair_produce<G, true, FULL, INVD, SLIM, PB6, DW6, SLOT>(a, img, sp, f, pk, last, more, stash, k, aa.ncoup, ybar, lbar, lbar_const, tile, nt, tile < ntiles, l31, hi, it & 1, tr);
        };
        // the first NF_PAIR_PARK rounds with their parked registers (one body per slot), the rest through memory
        int it0 = 0;
        if constexpr (!INVD) {
          static_assert(NF_PAIR_PARK == 2, "one call per slot");
          if (rounds > 0) produce(0, std::integral_constant<int, 0>{});
          if (rounds > 1) produce(1, std::integral_constant<int, 1>{});
          it0 = NF_PAIR_PARK;
        }
#pragma unroll 1
        for (int it = it0; it < rounds; ++it) produce(it, std::integral_constant<int, -1>{});
        NF_STAMP(trb, 3);
        __syncthreads();  // every wave is done with the weight image and the delta tiles
        NF_STAMP(trb, 4);
        // s and u of the next phase-S's first tile fly behind the fold, the slab write and the staging of the next image
        if (tile0 < ntiles) {
          if (!INVD && !is_s) stash_issue_first<G, SLIM>(f, stash, k, aa.ncoup, tile0, l31, hi);
          if (INVD && !is_s && step + 1 < aa.ncoup) stash_issue_first<G, SLIM>(f, stash, k - 1, aa.ncoup, tile0, l31, hi);
        }
        __syncthreads();  // the consumers have folded
        NF_STAMP(trb, 5);
        pair_slab_write<G>(lds, slab + (long)k * 2 * G::SIZE + ((long)blockIdx.x * slab_stride + (is_s ? 0 : 1) * (long)G::SIZE), tid);
        NF_STAMP(trb, 6);
        __syncthreads();
        NF_STAMP(trb, 7);
      }
    }
  } else {
#pragma unroll 1
    for (int step = 0; step < aa.ncoup; ++step) {
      const int k = INVD ? aa.ncoup - 1 - step : step;
      const float *img_s = aa.wimg + (size_t)(2 * k) * G::SIZE;
#pragma unroll 1
      for (int phase = 0; phase < 2; ++phase) {
        const bool is_s = INVD ? phase == 0 : phase == 1;
#ifdef NF_KERNEL_TRACE
        long long *trb = (aa.trace && blockIdx.x == 0 && tid == 256 + 64 * NF_TRACE_PAIR && step == 0) ? aa.trace + 96 + phase * 8 : nullptr;
#endif
        NF_STAMP(trb, 0);
        stage_image(k, is_s);
        NF_STAMP(trb, 1);
        __syncthreads();
        NF_STAMP(trb, 2);
        BwdAcc<G> acc;
        net_zero_acc(acc.w1, acc.b1);
        net_zero_acc(acc.w2, acc.b2);
        net_zero_acc(acc.w3, acc.b3);
#pragma unroll 1
        for (int it = 0; it < rounds; ++it) {
          const long tile = tile0 + (long)it * tstride;
#ifdef NF_KERNEL_TRACE  // consumer stamps at [64 + ...]
          long long *tr = (aa.trace && blockIdx.x == 0 && tid == 256 + 64 * NF_TRACE_PAIR && step == 0 && it < 2) ? aa.trace + 64 + phase * 16 + it * 8 : nullptr;
#else
          long long *tr = nullptr;
#endif
          pair_consume<G, SLIM, PB6, DW6>(img, sp, acc, stash, k, aa.ncoup, tile, is_s, tile < ntiles, l31, hi, it & 1, tr);
        }
        NF_STAMP(trb, 3);
        __syncthreads();  // every wave is done with the weight image and the delta tiles
        NF_STAMP(trb, 4);
        {
          float *mine = lds + pair * G::SIZE;
          fold_acc(mine + G::W1, mine + G::B1, acc.w1, acc.b1, true, l31, hi);
          fold_acc(mine + G::W2, mine + G::B2, acc.w2, acc.b2, true, l31, hi);
          fold_acc(mine + G::W3, mine + G::B3, acc.w3, acc.b3, true, l31, hi);
        }
        __syncthreads();
        NF_STAMP(trb, 5);
        pair_slab_write<G>(lds, slab + (long)k * 2 * G::SIZE + ((long)blockIdx.x * slab_stride + (is_s ? 0 : 1) * (long)G::SIZE), tid);
        NF_STAMP(trb, 6);
        __syncthreads();
        NF_STAMP(trb, 7);
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// host-side dispatch
// ------------------------------------------------------------------------------------
static inline int blocks32(int n) { return (n + 31) / 32; }
#define NF_GEO_H32 NetGeo<1, 1, 1, 1>
#define NF_GEO_H64 NetGeo<1, 2, 2, 1>

static int geo_size(const nf_flow_desc *desc) {
  if (desc->n_hidden != 2) return 0;
  const int c = (desc->d + 1) / 2;
  const int mb = blocks32(c), h1b = blocks32(desc->hdims[0]), h2b = blocks32(desc->hdims[1]);
  if (mb == 1 && h1b == 1 && h2b == 1) return NetGeo<1, 1, 1, 1>::SIZE;
  if (mb == 1 && h1b == 2 && h2b == 2) return NetGeo<1, 2, 2, 1>::SIZE;
  return 0;
}

// floats of one workgroup's gradient slab (image layout): [coupling][net s|t][G::SIZE]
long nf_affine_slab_floats(const nf_flow_desc *desc) {
  if (nf_deep_geo_id(desc)) return nf_deep_slab_floats(desc);
  return (long)2 * desc->nlayers * 2 * geo_size(desc);
}

int nf_affine_reduce_slabs(nf_ctx *ctx, const nf_flow_desc *desc, const float *slab, int nslab, float *g,
                           const double *lpart, int nlpart, float *lout) {
  if (nf_deep_geo_id(desc)) return nf_deep_reduce_slabs(ctx, desc, slab, nslab, g, lpart, nlpart, lout);
  const int size = geo_size(desc);
  if (!size) return NF_ERR_UNSUPPORTED;
  const PackArgs p = make_pack_args(desc);
  const long total = (long)p.ncoup * 2 * size;
  const unsigned grid = (unsigned)((total + 63) / 64);  // 64 elements per block (k_reduce_image_slabs)
  ProfScope ps(ctx, "reduce_slabs");
  if (size == NetGeo<1, 1, 1, 1>::SIZE)
    hipLaunchKernelGGL((k_reduce_image_slabs<NetGeo<1, 1, 1, 1>>), dim3(grid), dim3(64 * NF_REDUCE_WAVES), 0, ctx->stream, p, slab, nslab, total, g, lpart, nlpart, lout);
  else
    hipLaunchKernelGGL((k_reduce_image_slabs<NetGeo<1, 2, 2, 1>>), dim3(grid), dim3(64 * NF_REDUCE_WAVES), 0, ctx->stream, p, slab, nslab, total, g, lpart, nlpart, lout);
  return (int)hipGetLastError();
}

// the fused epilogue of nf_elbo_step (nf_pack.h: k_affine_epilogue).  mode: 1 = slabs -> gradient + loss only (multi-GPU,
// before the all-reduce), 2 = Adam + ||g|| + packed images from a finished gradient (after it), 3 = both (single GPU).
long nf_affine_epilogue_blocks(const nf_flow_desc *desc) { return ((long)2 * desc->nlayers * 2 * geo_size(desc) + 63) / 64; }
int nf_affine_epilogue(nf_ctx *ctx, const nf_flow_desc *desc, int mode, const float *slab, int nslab, float *g,
                       const double *lpart, int nlpart, float *theta, float *m, float *v, double lr, double b1, double b2,
                       double eps, unsigned t_val, unsigned *t_ptr, double *gpart) {
  const int size = geo_size(desc);
  if (!size || !ctx->wimg) return NF_ERR_UNSUPPORTED;
  const PackArgs p = make_pack_args(desc);
  EpiArgs a;
  a.slab = slab; a.nslab = nslab; a.slab_stride = (long)p.ncoup * 2 * size;
  a.g = g; a.P = nf_param_count(desc);
  a.lpart = lpart; a.nlpart = nlpart;
  a.theta = theta; a.m = m; a.v = v; a.wimg = (float *)ctx->wimg;
  a.lr = (float)lr; a.b1 = (float)b1; a.b2 = (float)b2; a.eps = (float)eps; a.b1d = b1; a.b2d = b2;
  a.t_val = t_val; a.t_ptr = t_ptr; a.gpart = gpart;
  a.c1 = (float)(1.0 - pow(b1, (double)t_val + 1.0));
  a.c2 = (float)(1.0 - pow(b2, (double)t_val + 1.0));
  const unsigned grid = (unsigned)nf_affine_epilogue_blocks(desc);
  if (mode != 1) ctx->wimg_gen++;  // the fp32 images are rewritten (Adam's theta): B6 copies are stale
  // (Measured and removed, twice: the epilogue refreshing the B6T images element by element as well, which saves the next step its
  // conversion launch.  First with one thread per 16-byte row -- the reverse kernel then stages images that were written a whole
  // forward kernel earlier instead of a moment ago and runs 4-5 us slower: 0.594 against 0.594 ms per step.  Then in the Adam
  // thread's own index, a quad of lanes gathering 8 bytes per part: 0.5665 [0.5652-0.5693] against 0.5655 [0.5646-0.5707] ms,
  // five alternating pairs on one box (profiles/cotangent_carry_ab.txt).)
  ProfScope ps(ctx, mode == 2 ? "adam" : "reduce_slabs");
  const bool h64 = size != NetGeo<1, 1, 1, 1>::SIZE;
#define NF_EPI(GEO)                                                                                                          \
  do {                                                                                                                       \
    if (mode == 3) hipLaunchKernelGGL((k_affine_epilogue<GEO, true, true, NF_REDUCE_WAVES>), dim3(grid), dim3(64 * NF_REDUCE_WAVES), 0, ctx->stream, p, a); \
    else if (mode == 1) hipLaunchKernelGGL((k_affine_epilogue<GEO, true, false, NF_REDUCE_WAVES>), dim3(grid), dim3(64 * NF_REDUCE_WAVES), 0, ctx->stream, p, a); \
    else hipLaunchKernelGGL((k_affine_epilogue<GEO, false, true, 1>), dim3(grid), dim3(64), 0, ctx->stream, p, a);             \
  } while (0)
  if (h64) NF_EPI(NF_GEO_H64); else NF_EPI(NF_GEO_H32);
#undef NF_EPI
  return (int)hipGetLastError();
}

// packs every net of the flow into ctx->wimg (grow-only) -- call once per API entry
// Where the B6 images sit: behind the fp32 images of the same flow in ctx->wimg (nf_affine_wimg_bytes covers both).
template <class G>
static size_t b6_offset_bytes(const nf_flow_desc *desc) { return (size_t)2 * desc->nlayers * 2 * G::SIZE * sizeof(float); }
// Which chain launches take the bf16 six-term products (B6).  Measured A/B on one box (profiles/r4i_b6_ab.txt):
//   * chains WITHOUT a stash (nf_flow_fwd / nf_flow_inv, nf_elbo_batch, nf_loglikelihood: BASELINE cfg 5, 1 M samples):
//     1.69 against 2.46 ms = 1.45 x, 620 M samples/s, 1.03 of the fp32-MFMA roofline -- ON by default, NF_FWD_FP32=1 is the
//     A/B switch back;
//   * the training step's stashing forward (cfg 2): 207-210 against 195 us, AND the unchanged reverse kernel behind it runs
//     400 instead of 362 us (the chip's power management couples consecutive kernels: tools/bench_ramp.py shows the clock is
//     set by the load of the last milliseconds) -- 0.659 against 0.612 ms per step: OFF by default, NF_FWD_B6_STASH=1 turns
//     it on (120 bytes of scratch spills in that variant are the first thing to remove).
static bool fwd_b6(bool stashing = false) {
  static const bool off = std::getenv("NF_FWD_FP32") != nullptr, stash_on = std::getenv("NF_FWD_B6_STASH") != nullptr;
  return !off && (!stashing || stash_on);
}

static size_t b6_image_bytes(int size) { return size == NetGeo<1, 1, 1, 1>::SIZE ? B6Geo<NetGeo<1, 1, 1, 1>>::BYTES : B6Geo<NetGeo<1, 2, 2, 1>>::BYTES; }
static size_t b6t_image_bytes(int size) { return size == NetGeo<1, 1, 1, 1>::SIZE ? B6TGeo<NetGeo<1, 1, 1, 1>>::BYTES : B6TGeo<NetGeo<1, 2, 2, 1>>::BYTES; }
// ctx->wimg of a resident RealNVP flow: [fp32 images][B6 images (forward chain)][B6T images (pair kernel's dX GEMMs)]
size_t nf_affine_wimg_bytes(const nf_flow_desc *desc) {
  if (nf_deep_geo_id(desc)) return nf_deep_wimg_bytes(desc);
  const int size = geo_size(desc);
  return (size_t)2 * desc->nlayers * 2 * ((size_t)size * sizeof(float) + (size ? b6_image_bytes(size) + b6t_image_bytes(size) : 0));
}
template <class G>
static size_t b6t_offset_bytes(const nf_flow_desc *desc) { return b6_offset_bytes<G>(desc) + (size_t)2 * desc->nlayers * 2 * B6Geo<G>::BYTES; }
template <class G>
static int b6t_refresh(nf_ctx *ctx, const nf_flow_desc *desc) {
  if (ctx->b6t_gen == ctx->wimg_gen) return NF_OK;
  using B = B6TGeo<G>;
  const int nimg = 2 * desc->nlayers * 2;
  constexpr long PER = 2 * G::CB * 2 * B::R3 + 2 * G::H2B * 2 * B::R2 + 2 * G::H1B * 2 * B::R1;
  const long total = (long)nimg * PER;
  ProfScope ps(ctx, "pack_weights");
  hipLaunchKernelGGL((k_b6t_from_images<G>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, nimg, (const float *)ctx->wimg,
                     (unsigned char *)ctx->wimg + b6t_offset_bytes<G>(desc));
  NF_HIP(hipGetLastError());
  ctx->b6t_gen = ctx->wimg_gen;
  return NF_OK;
}

// the bf16-triple images of the chain kernels that use the six-term products (B6), rebuilt from the fp32 images when those
// have been rewritten since (ctx->wimg_gen): behind the fp32 images in ctx->wimg
template <class G>
static int b6_refresh(nf_ctx *ctx, const nf_flow_desc *desc) {
  if (ctx->b6_gen == ctx->wimg_gen) return NF_OK;
  using B = B6Geo<G>;
  const int nimg = 2 * desc->nlayers * 2;
  constexpr long PER = 2 * G::MB * 2 * B::R1 + 2 * G::H1B * 2 * B::R2 + 2 * G::H2B * 2 * B::R3 + B::R1 + B::R2 + B::R3;
  const long total = (long)nimg * PER;
  ProfScope ps(ctx, "pack_weights");
  hipLaunchKernelGGL((k_b6_from_images<G>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, nimg, (const float *)ctx->wimg,
                     (unsigned char *)ctx->wimg + b6_offset_bytes<G>(desc));
  NF_HIP(hipGetLastError());
  ctx->b6_gen = ctx->wimg_gen;
  return NF_OK;
}

int nf_affine_pack(nf_ctx *ctx, const nf_flow_desc *desc, const float *theta) {
  if (nf_deep_geo_id(desc)) return nf_deep_pack(ctx, desc, theta);
  if (desc->n_hidden != 2) return NF_ERR_UNSUPPORTED;
  const int size = geo_size(desc);
  if (!size) return NF_ERR_UNSUPPORTED;
  const int nc = 2 * desc->nlayers;
  NF_TRY(nf_wimg_reserve(ctx, nf_affine_wimg_bytes(desc)));
  const PackArgs p = make_pack_args(desc);
  const long total = (long)nc * 2 * size;
  const unsigned grid = (unsigned)((total + 255) / 256);
  {
    ProfScope ps(ctx, "pack_weights");
    if (size == NetGeo<1, 1, 1, 1>::SIZE)
      hipLaunchKernelGGL((k_pack_net_images<NetGeo<1, 1, 1, 1>>), dim3(grid), dim3(256), 0, ctx->stream, p, theta, (float *)ctx->wimg);
    else
      hipLaunchKernelGGL((k_pack_net_images<NetGeo<1, 2, 2, 1>>), dim3(grid), dim3(256), 0, ctx->stream, p, theta, (float *)ctx->wimg);
    NF_HIP(hipGetLastError());
  }
  return NF_OK;
}

static int make_args(nf_ctx *ctx, const nf_flow_desc *desc, int k, const float *theta, long N, CouplingArgs *out) {
  if (desc->n_hidden != 2) return NF_ERR_UNSUPPORTED;
  CouplingInfo ci = nf_coupling_info(desc, k);
  CouplingArgs a;
  a.theta = theta;
  const int size = geo_size(desc);
  if (!size || !ctx->wimg) return NF_ERR_UNSUPPORTED;
  a.img_s = (const float *)ctx->wimg + (size_t)(2 * k) * size;
  a.img_t = a.img_s + size;
  a.trace = (long long *)ctx->trace;
  a.d = desc->d; a.c = ci.c; a.m = ci.m; a.par_t = ci.par_t; a.N = N;
  const int h1 = desc->hdims[0], h2 = desc->hdims[1];
  a.s = make_net_dims(ci.theta_off, ci.m, h1, h2, ci.c);
  a.t = make_net_dims(ci.theta_off + net_param_count(ci.m, h1, h2, ci.c), ci.m, h1, h2, ci.c);
  *out = a;
  return NF_OK;
}

#define NF_GEO_DISPATCH(MBv, H1v, H2v, CBv, BODY)                          \
  if (mb == MBv && h1b == H1v && h2b == H2v && cb == CBv) {                 \
    using G = NetGeo<MBv, H1v, H2v, CBv>;                                   \
    BODY                                                                    \
  }

template <class G, bool INV, bool FULL>
static int launch_apply_v(nf_ctx *ctx, const CouplingArgs &a, const float *x, float *y, float *ladj, int accumulate) {
  const size_t lds = 2 * (size_t)G::SIZE * sizeof(float);
  NF_TRY((nf_lds_once<k_affine_apply<G, INV, FULL>>(ctx, lds)));
  const long ntiles = (a.N + NF_TILE - 1) / NF_TILE;
  long grid = (ntiles + 7) / 8;
  const long cap = 2L * ctx->num_cu;
  if (grid > cap) grid = cap;
  if (grid < 1) grid = 1;
  ProfScope ps(ctx, "affine_apply");
  hipLaunchKernelGGL((k_affine_apply<G, INV, FULL>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a, x, y, ladj, accumulate);
  return (int)hipGetLastError();
}
template <class G, bool INV>
static int launch_apply(nf_ctx *ctx, const CouplingArgs &a, const float *x, float *y, float *ladj, int accumulate) {
  const bool full = a.m == 32 * G::MB && a.c == 32 * G::CB && a.N % NF_TILE == 0;
  return full ? launch_apply_v<G, INV, true>(ctx, a, x, y, ladj, accumulate)
              : launch_apply_v<G, INV, false>(ctx, a, x, y, ladj, accumulate);
}

// in place, on the six-term products: what the whole-chain launch of the same flow computes for this coupling
template <class G>
static int launch_apply_b6(nf_ctx *ctx, const nf_flow_desc *desc, int k, bool inverse, const CouplingArgs &a, float *xy, float *ladj,
                           int accumulate) {
  using BG = B6Geo<G>;
  const size_t lds = 2 * (size_t)BG::BYTES;
  static AttrOnce attr_once;  // once per device: a context on another GPU needs its own
  NF_TRY(attr_once.run(ctx->device, [&]() -> int {
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_apply_b6<G, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_apply_b6<G, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return NF_OK;
  }));
  NF_TRY(b6_refresh<G>(ctx, desc));
  const unsigned char *img6 = (const unsigned char *)ctx->wimg + b6_offset_bytes<G>(desc) + (size_t)(2 * k) * BG::BYTES;
  const long ntiles = (a.N + NF_TILE - 1) / NF_TILE;
  long grid = (ntiles + 7) / 8;
  const long cap = 2L * ctx->num_cu;
  if (grid > cap) grid = cap;
  if (grid < 1) grid = 1;
  ProfScope ps(ctx, "affine_apply");
  if (inverse)
    hipLaunchKernelGGL((k_affine_apply_b6<G, true>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a, img6, xy, ladj, accumulate);
  else
    hipLaunchKernelGGL((k_affine_apply_b6<G, false>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a, img6, xy, ladj, accumulate);
  return (int)hipGetLastError();
}

int nf_affine_apply(nf_ctx *ctx, const nf_flow_desc *desc, int k, bool inverse, const float *theta, const float *x,
                    long N, float *y, float *ladj, int accumulate) {
  if (nf_deep_geo_id(desc)) {
    if (x != y) return NF_ERR_UNSUPPORTED;  // (every caller applies a coupling in place on the tiled buffer)
    return nf_deep_chain(ctx, desc, inverse, y, N, ladj, k, accumulate);
  }
  CouplingArgs a;
  NF_TRY(make_args(ctx, desc, k, theta, N, &a));
  const int mb = blocks32(a.m > a.c ? a.m : a.c), h1b = blocks32(desc->hdims[0]), h2b = blocks32(desc->hdims[1]), cb = mb;
  if (x == y && fwd_b6()) {  // the arithmetic nf_affine_chain uses for the whole flow (NF_FWD_FP32: the fp32 kernels below, as there)
#define BODY_APPLY6 return launch_apply_b6<G>(ctx, desc, k, inverse, a, y, ladj, accumulate);
    NF_GEO_DISPATCH(1, 1, 1, 1, BODY_APPLY6)
    NF_GEO_DISPATCH(1, 2, 2, 1, BODY_APPLY6)
#undef BODY_APPLY6
  }
#define BODY_APPLY                                                              \
  return inverse ? launch_apply<G, true>(ctx, a, x, y, ladj, accumulate)        \
                 : launch_apply<G, false>(ctx, a, x, y, ladj, accumulate);
  NF_GEO_DISPATCH(1, 1, 1, 1, BODY_APPLY)
  NF_GEO_DISPATCH(1, 2, 2, 1, BODY_APPLY)
#undef BODY_APPLY
  return NF_ERR_UNSUPPORTED;
}

template <class G, bool FULL>
static int launch_bwd_v(nf_ctx *ctx, const CouplingArgs &a, float *y, float *ybar, const float *lbar, float lbar_const,
                        float *slab, long slab_stride, int grid) {
  const size_t lds = BwdLds<G>::BYTES;
  NF_TRY((nf_lds_once<k_affine_bwd<G, FULL>>(ctx, lds)));
  ProfScope ps(ctx, "affine_bwd");
  hipLaunchKernelGGL((k_affine_bwd<G, FULL>), dim3((unsigned)grid), dim3(256), lds, ctx->stream, a, y, ybar, lbar,
                     lbar_const, slab, slab_stride);
  return (int)hipGetLastError();
}
// Which stash layout the training step of this flow uses (forward writer and reverse reader must agree).  SLIM is OFF by
// default: measured A/B in one process on one box (cfg 2, driver's command, profiles/r4c_stash_slim_ab.txt) the forward gains
// 4 us of 199 (it is issue-bound, not write-bound: 124 fewer store instructions per coupling buy 2 %), the reverse kernel
// LOSES 52 us of 369 -- the 32 extra MFMAs per net and tile do not hide in the consumer's prologue, they wait there for x2 --
// 0.730 against 0.691 ms per step.  NF_STASH_SLIM=1 selects it where the two-waves-per-tile kernel reads the stash (hidden
// 33-64): 26 % less stash memory and HBM traffic for 5 % more time.
static bool stash_slim(int size) {
  static const bool no_pair = std::getenv("NF_BWD_NO_PAIR") != nullptr, slim = std::getenv("NF_STASH_SLIM") != nullptr;
  return size == NetGeo<1, 2, 2, 1>::SIZE && !no_pair && slim;
}

template <class G, bool SLIM = false, bool B6 = false>
static int launch_chain(nf_ctx *ctx, const nf_flow_desc *desc, bool inverse, float *xt, long N, float *ladj,
                        const FusedArgs *fused = nullptr, float *stash_plain = nullptr) {
  // two double-buffered (s,t) image pairs (B6: three single images) + target parameters and per-wave sums of the fused variant
  const size_t lds = (B6 ? (size_t)3 * B6Geo<G>::BYTES : 4 * (size_t)G::SIZE * sizeof(float)) + (2 * 64 * G::CB + 2) * sizeof(float) +
                     12 * sizeof(double);
  // k_affine_chain_tgt (the fused forward for the Banana / Funnel / WarpedGauss / Cross targets): eight waves per workgroup
  // where the instantiation fits 256 registers without scratch, four (one per SIMD, 512 registers) where it does not -- the
  // six-term forms at hidden 64 without a stash (44 bytes at eight) and with the slim stash (12 bytes); by
  // tools/kernel_resources.py, held by tests/test_elbo_targets_cpu.py.  The grid does not depend on it (the tile-group loop strides).
  constexpr bool H64G = G::H1B == 2;
  constexpr int NWT_S = (H64G && B6 && SLIM) ? 4 : 8, NWT_P = (H64G && B6) ? 4 : 8;
  static AttrOnce attr_once;  // once per device: a context on another GPU needs its own
  NF_TRY(attr_once.run(ctx->device, [&]() -> int {
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain<G, false, false, false, false, B6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain<G, true, false, false, false, B6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain<G, false, true, false, false, B6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain<G, false, true, true, SLIM, B6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain<G, false, false, true, SLIM, B6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain<G, true, false, true, SLIM, B6>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain_tgt<G, true, SLIM, B6, NWT_S>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_chain_tgt<G, false, false, B6, NWT_P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return NF_OK;
  }));
  if (B6) NF_TRY(b6_refresh<G>(ctx, desc));
  ChainArgs a;
  a.wimg = (const float *)ctx->wimg;
  a.wimg_b6 = (const unsigned char *)ctx->wimg + b6_offset_bytes<G>(desc);
  a.d = desc->d;
  a.ncoup = 2 * desc->nlayers;
  a.N = N;
  const long ngroups = ((N + NF_TILE - 1) / NF_TILE + 7) / 8;
  long grid = ngroups < ctx->num_cu ? ngroups : ctx->num_cu;
  if (grid < 1) grid = 1;
  const bool tgt = fused && fused->tkind != NF_TARGET_DIAGGAUSS;  // the other built-in targets: k_affine_chain_tgt, profiled under its own name
  ProfScope ps(ctx, tgt ? "affine_chain_tgt" : "affine_chain");
  FusedArgs none{};
  none.trace = (long long *)ctx->trace;
  if (tgt && fused->stash)
    hipLaunchKernelGGL((k_affine_chain_tgt<G, true, SLIM, B6, NWT_S>), dim3((unsigned)grid), dim3(64 * NWT_S), lds, ctx->stream, a, xt, *fused);
  else if (tgt)
    hipLaunchKernelGGL((k_affine_chain_tgt<G, false, false, B6, NWT_P>), dim3((unsigned)grid), dim3(64 * NWT_P), lds, ctx->stream, a, xt, *fused);
  else if (fused && fused->stash)
    hipLaunchKernelGGL((k_affine_chain<G, false, true, true, SLIM, B6>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a, xt, ladj, *fused);
  else if (fused)
    hipLaunchKernelGGL((k_affine_chain<G, false, true, false, false, B6>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a, xt, ladj, *fused);
  else if (inverse && stash_plain) {  // forward-KL training: the inverse chain leaves the stash of ITS reverse pass
    none.stash = stash_plain;
    hipLaunchKernelGGL((k_affine_chain<G, true, false, true, SLIM, B6>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a, xt, ladj, none);
  } else if (inverse) {
    const long g8 = ((N + NF_TILE - 1) / NF_TILE + 7) / 8;
    const long gridp = g8 < 1 ? 1 : g8 < ctx->num_cu ? g8 : ctx->num_cu;
    hipLaunchKernelGGL((k_affine_chain<G, true, false, false, false, B6>), dim3((unsigned)gridp), dim3(512), lds, ctx->stream, a, xt, ladj, none);
  } else if (stash_plain) {  // caller-supplied draws: the plain forward chain, leaving the stash behind
    none.stash = stash_plain;
    hipLaunchKernelGGL((k_affine_chain<G, false, false, true, SLIM, B6>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, a, xt, ladj, none);
  } else {
    const long g8 = ((N + NF_TILE - 1) / NF_TILE + 7) / 8;
    const long gridp = g8 < 1 ? 1 : g8 < ctx->num_cu ? g8 : ctx->num_cu;
    hipLaunchKernelGGL((k_affine_chain<G, false, false, false, false, B6>), dim3((unsigned)gridp), dim3(512), lds, ctx->stream, a, xt, ladj, none);
  }
  return (int)hipGetLastError();
}

// number of workgroups (= entries of `partial`) the fused ELBO-forward launch uses
long nf_affine_chain_grid(nf_ctx *ctx, long N) {
  const long ngroups = ((N + NF_TILE - 1) / NF_TILE + 7) / 8;
  long grid = ngroups < ctx->num_cu ? ngroups : ctx->num_cu;
  return grid < 1 ? 1 : grid;
}

// base draws + whole chain forward + built-in target + ELBO partial sums in one launch
// (packed images must be current).  yt <- flow output (tiled; may be null WITH a stash: the output is then not written, the
// stashed reverse pass does not read it), gt <- gscale * grad log p(y) (or null),
// partial[nf_affine_chain_grid] <- sums of pscale * elbo_j.  The diagonal Gaussian runs k_affine_chain<FUSED>, the other
// four kinds k_affine_chain_tgt; WarpedGauss / Cross with d != 2 and a diagonal Gaussian without parameters are refused here.
int nf_affine_chain_elbo(nf_ctx *ctx, const nf_flow_desc *desc, long N, uint64_t seed, uint64_t off, uint32_t stream,
                         const nf_target *target, float *yt, float *gt, double gscale, double *partial,
                         double pscale, float *stash, const uint32_t *stream_ptr) {
  const int size = geo_size(desc);
  if (!size || !ctx->wimg) return NF_ERR_UNSUPPORTED;
  if (!yt && !stash) return NF_ERR_ARG;
  NF_TRY(nf_target_check(target, desc->d));
  const float *mu = (const float *)target->p0, *var = (const float *)target->p1;
  FusedArgs fa;
  fa.tkind = target->kind; fa.ts0 = (float)target->s0; fa.ts1 = (float)target->s1;
  fa.stash = stash;
  fa.trace = (long long *)ctx->trace;
  fa.stream_ptr = stream_ptr;
  fa.k0 = (uint32_t)seed; fa.k1 = (uint32_t)(seed >> 32); fa.stream = stream; fa.off = off;
  fa.mu = mu; fa.var = var; fa.gt = gt; fa.gscale = (float)gscale; fa.partial = partial; fa.pscale = pscale;
  const bool b6 = fwd_b6(stash != nullptr);
  if (size == NetGeo<1, 1, 1, 1>::SIZE)
    return b6 ? launch_chain<NetGeo<1, 1, 1, 1>, false, true>(ctx, desc, false, yt, N, nullptr, &fa)
              : launch_chain<NetGeo<1, 1, 1, 1>>(ctx, desc, false, yt, N, nullptr, &fa);
  if (stash && stash_slim(size))
    return b6 ? launch_chain<NetGeo<1, 2, 2, 1>, true, true>(ctx, desc, false, yt, N, nullptr, &fa)
              : launch_chain<NetGeo<1, 2, 2, 1>, true>(ctx, desc, false, yt, N, nullptr, &fa);
  return b6 ? launch_chain<NetGeo<1, 2, 2, 1>, false, true>(ctx, desc, false, yt, N, nullptr, &fa)
            : launch_chain<NetGeo<1, 2, 2, 1>>(ctx, desc, false, yt, N, nullptr, &fa);
}

// whole chain in one launch, in place on the tiled buffer (packed images must be current)
int nf_affine_chain(nf_ctx *ctx, const nf_flow_desc *desc, bool inverse, float *xt, long N, float *ladj, float *stash) {
  if (nf_deep_geo_id(desc)) return stash ? NF_ERR_UNSUPPORTED : nf_deep_chain(ctx, desc, inverse, xt, N, ladj, -1, 0);
  const int size = geo_size(desc);
  if (!size || !ctx->wimg) return NF_ERR_UNSUPPORTED;
  const bool b6 = fwd_b6(stash != nullptr);
  if (size == NetGeo<1, 1, 1, 1>::SIZE)
    return b6 ? launch_chain<NetGeo<1, 1, 1, 1>, false, true>(ctx, desc, inverse, xt, N, ladj, nullptr, stash)
              : launch_chain<NetGeo<1, 1, 1, 1>>(ctx, desc, inverse, xt, N, ladj, nullptr, stash);
  if (stash && stash_slim(size))
    return b6 ? launch_chain<NetGeo<1, 2, 2, 1>, true, true>(ctx, desc, inverse, xt, N, ladj, nullptr, stash)
              : launch_chain<NetGeo<1, 2, 2, 1>, true>(ctx, desc, inverse, xt, N, ladj, nullptr, stash);
  return b6 ? launch_chain<NetGeo<1, 2, 2, 1>, false, true>(ctx, desc, inverse, xt, N, ladj, nullptr, stash)
            : launch_chain<NetGeo<1, 2, 2, 1>>(ctx, desc, inverse, xt, N, ladj, nullptr, stash);
}

// The forward-KL training step's inverse chain (nf_loglikelihood_step): ys (d x N, standard layout, read in place) -> every
// coupling inverse with its stash, gt <- gscale * grad log q0(z) (tiled) and partial[nf_affine_chain_grid] <- sums of
// pscale * (log q0(z_j) + ladj_inv_j), in one launch (packed images must be current).  It has the stash writer of the default
// split sequence (fp32 MFMAs, full stash layout); under the A/B switches NF_FWD_B6_STASH / NF_STASH_SLIM that sequence writes
// another stash, and the step keeps it.
bool nf_affine_chain_fkl_ok(const nf_flow_desc *desc) {
  if (nf_deep_geo_id(desc)) return false;
  const int size = geo_size(desc);
  return size && !fwd_b6(true) && !stash_slim(size);
}
template <class G>
static int launch_chain_fkl(nf_ctx *ctx, const nf_flow_desc *desc, const float *ys, long N, const FusedArgs &fa) {
  const size_t lds = 4 * (size_t)G::SIZE * sizeof(float) + (2 * 64 * G::CB + 2) * sizeof(float) + 12 * sizeof(double);
  NF_TRY((nf_lds_once<k_affine_chain<G, true, true, true>>(ctx, lds)));
  ChainArgs a;
  a.wimg = (const float *)ctx->wimg;
  a.wimg_b6 = nullptr;
  a.d = desc->d;
  a.ncoup = 2 * desc->nlayers;
  a.N = N;
  ProfScope ps(ctx, "affine_chain_fkl");
  hipLaunchKernelGGL((k_affine_chain<G, true, true, true>), dim3((unsigned)nf_affine_chain_grid(ctx, N)), dim3(512), lds, ctx->stream, a,
                     const_cast<float *>(ys), nullptr, fa);
  return (int)hipGetLastError();
}
int nf_affine_chain_fkl(nf_ctx *ctx, const nf_flow_desc *desc, const float *ys, long N, float *gt, double gscale, double *partial,
                        double pscale, float *stash) {
  if (!nf_affine_chain_fkl_ok(desc) || !ctx->wimg || !stash) return NF_ERR_UNSUPPORTED;
  if (N <= 0) return NF_OK;
  FusedArgs fa{};
  fa.trace = (long long *)ctx->trace;
  fa.gt = gt; fa.gscale = (float)gscale; fa.partial = partial; fa.pscale = pscale; fa.stash = stash;
  if (geo_size(desc) == NetGeo<1, 1, 1, 1>::SIZE) return launch_chain_fkl<NetGeo<1, 1, 1, 1>>(ctx, desc, ys, N, fa);
  return launch_chain_fkl<NetGeo<1, 2, 2, 1>>(ctx, desc, ys, N, fa);
}

template <class G>
static int launch_bwd(nf_ctx *ctx, const CouplingArgs &a, float *y, float *ybar, const float *lbar, float lbar_const,
                      float *slab, long slab_stride, int grid) {
  const bool full = a.m == 32 * G::MB && a.c == 32 * G::CB && a.N % NF_TILE == 0;
  return full ? launch_bwd_v<G, true>(ctx, a, y, ybar, lbar, lbar_const, slab, slab_stride, grid)
              : launch_bwd_v<G, false>(ctx, a, y, ybar, lbar, lbar_const, slab, slab_stride, grid);
}

// number of workgroups (= partial-gradient slabs) the reverse pass uses for a batch of N
int nf_affine_bwd_grid(nf_ctx *ctx, long N) {
  const long ntiles = (N + NF_TILE - 1) / NF_TILE;
  long grid = (ntiles + 3) / 4;
  if (grid > ctx->num_cu) grid = ctx->num_cu;
  if (grid < 1) grid = 1;
  return (int)grid;
}

int nf_affine_bwd(nf_ctx *ctx, const nf_flow_desc *desc, int k, const float *theta, float *y, float *ybar,
                  const float *lbar, float lbar_const, long N, float *slab, long slab_stride, int grid) {
  if (nf_deep_geo_id(desc)) return nf_deep_bwd(ctx, desc, k, k + 1, y, ybar, lbar, lbar_const, N, slab, slab_stride, grid, false);
  CouplingArgs a;
  NF_TRY(make_args(ctx, desc, k, theta, N, &a));
  const int mb = blocks32(a.m > a.c ? a.m : a.c), h1b = blocks32(desc->hdims[0]), h2b = blocks32(desc->hdims[1]), cb = mb;
#define BODY_BWD return launch_bwd<G>(ctx, a, y, ybar, lbar, lbar_const, slab + (long)k * 2 * G::SIZE, slab_stride, grid);
  NF_GEO_DISPATCH(1, 1, 1, 1, BODY_BWD)
  NF_GEO_DISPATCH(1, 2, 2, 1, BODY_BWD)
#undef BODY_BWD
  return NF_ERR_UNSUPPORTED;
}

template <class G, bool FULL, bool INVD = false>
static int launch_bwd_all_v(nf_ctx *ctx, const BwdAllArgs &aa, float *y, float *ybar, const float *lbar, float lbar_const,
                            float *slab, long slab_stride, int grid) {
  const size_t lds = BwdLds<G>::BYTES;
  NF_TRY((nf_lds_once<k_affine_bwd_all<G, FULL, INVD>>(ctx, lds)));
  ProfScope ps(ctx, INVD ? "affine_bwd_inv" : "affine_bwd");
  hipLaunchKernelGGL((k_affine_bwd_all<G, FULL, INVD>), dim3((unsigned)grid), dim3(256), lds, ctx->stream, aa, y, ybar, lbar,
                     lbar_const, slab, slab_stride);
  return (int)hipGetLastError();
}

// reverse pass of ALL couplings in one launch (flat order = reverse of execution order); packed images
// must be current.  Slab layout as with nf_affine_bwd called for k = 0 .. ncoup-1.
// inv_dir: reverse pass of the INVERSE chain instead (y: T^-1(data) -> data, couplings in execution order).
int nf_affine_bwd_all(nf_ctx *ctx, const nf_flow_desc *desc, float *y, float *ybar, const float *lbar, float lbar_const,
                      long N, float *slab, long slab_stride, int grid, bool inv_dir) {
  if (nf_deep_geo_id(desc)) return nf_deep_bwd(ctx, desc, 0, 2 * desc->nlayers, y, ybar, lbar, lbar_const, N, slab, slab_stride, grid, inv_dir);
  const int size = geo_size(desc);
  if (!size || !ctx->wimg || desc->n_hidden != 2) return NF_ERR_UNSUPPORTED;
  BwdAllArgs aa;
  aa.wimg = (const float *)ctx->wimg;
  aa.wimg_b6t = nullptr;
  aa.trace = (long long *)ctx->trace;
  aa.d = desc->d;
  aa.ncoup = 2 * desc->nlayers;
  aa.N = N;
  aa.no_xbar = 0;
  const bool h64 = size != NetGeo<1, 1, 1, 1>::SIZE;
  const bool full = desc->d == 64 && N % NF_TILE == 0;  // both partitions fill their 32-row block
  if (inv_dir) {
    if (h64)
      return full ? launch_bwd_all_v<NetGeo<1, 2, 2, 1>, true, true>(ctx, aa, y, ybar, lbar, lbar_const, slab, slab_stride, grid)
                  : launch_bwd_all_v<NetGeo<1, 2, 2, 1>, false, true>(ctx, aa, y, ybar, lbar, lbar_const, slab, slab_stride, grid);
    return launch_bwd_all_v<NetGeo<1, 1, 1, 1>, false, true>(ctx, aa, y, ybar, lbar, lbar_const, slab, slab_stride, grid);
  }
  if (h64)
    return full ? launch_bwd_all_v<NetGeo<1, 2, 2, 1>, true>(ctx, aa, y, ybar, lbar, lbar_const, slab, slab_stride, grid)
                : launch_bwd_all_v<NetGeo<1, 2, 2, 1>, false>(ctx, aa, y, ybar, lbar, lbar_const, slab, slab_stride, grid);
  return full ? launch_bwd_all_v<NetGeo<1, 1, 1, 1>, true>(ctx, aa, y, ybar, lbar, lbar_const, slab, slab_stride, grid)
              : launch_bwd_all_v<NetGeo<1, 1, 1, 1>, false>(ctx, aa, y, ybar, lbar, lbar_const, slab, slab_stride, grid);
}

// floats of the training step's activation stash (0: shape without a stash kernel)
size_t nf_affine_stash_floats(const nf_flow_desc *desc, long N) {
  const int size = geo_size(desc);
  if (!size || desc->n_hidden != 2) return 0;
  const size_t ntiles = (size_t)((N + NF_TILE - 1) / NF_TILE);
  const size_t per = size == NetGeo<1, 1, 1, 1>::SIZE ? StashGeo<NetGeo<1, 1, 1, 1>>::SIZE
                     : stash_slim(size) ? StashGeo<NetGeo<1, 2, 2, 1>, true>::SIZE : StashGeo<NetGeo<1, 2, 2, 1>>::SIZE;
  return ntiles * (size_t)(2 * desc->nlayers) * per;
}

// Is the stash the faster reverse pass for this shape?  Measured A/B on one box at batch 65 536, d = 64: hidden 64
// (NetGeo<1,2,2,1>) 0.667 vs 0.734 ms per step; hidden 32 (NetGeo<1,1,1,1>) 0.381 vs 0.370 ms -- the narrow nets' recompute
// is cheaper than their stash's HBM round trip, so there the stash is used only on request (nf_ctx_set_stash_budget > 0).
bool nf_affine_stash_pays(const nf_flow_desc *desc) { return geo_size(desc) == NetGeo<1, 2, 2, 1>::SIZE; }

template <class G, bool FULL, bool INVD = false>
static int launch_bwd_stashed_v(nf_ctx *ctx, const BwdAllArgs &aa0, float *stash, float *ybar, const float *lbar, float lbar_const,
                                float *slab, long slab_stride, int grid, const nf_flow_desc *desc = nullptr) {
  const size_t lds = BwdStashLds<G>::BYTES;
  static AttrOnce attr_once;  // once per device
  NF_TRY(attr_once.run(ctx->device, [&]() -> int {
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_bwd_stashed<G, FULL, INVD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    NF_HIP(hipFuncSetAttribute((const void *)k_affine_bwd_stashed<G, FULL, INVD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return NF_OK;
  }));
  // NF_BWD_ONE_WAVE_B6=1 (with NF_BWD_NO_PAIR=1 for hidden 33-64): every GEMM of the one-wave kernel on the bf16 matrix cores
  static const bool sb6 = std::getenv("NF_BWD_ONE_WAVE_B6") != nullptr;
  BwdAllArgs aa = aa0;
  ProfScope ps(ctx, INVD ? "affine_bwd_inv" : "affine_bwd");
  if (sb6 && desc) {
    NF_TRY(b6t_refresh<G>(ctx, desc));
    aa.wimg_b6t = (const unsigned char *)ctx->wimg + b6t_offset_bytes<G>(desc);
    hipLaunchKernelGGL((k_affine_bwd_stashed<G, FULL, INVD, true>), dim3((unsigned)grid), dim3(256), lds, ctx->stream, aa, stash, ybar, lbar,
                       lbar_const, slab, slab_stride);
  } else
    hipLaunchKernelGGL((k_affine_bwd_stashed<G, FULL, INVD>), dim3((unsigned)grid), dim3(256), lds, ctx->stream, aa, stash, ybar, lbar,
                       lbar_const, slab, slab_stride);
  return (int)hipGetLastError();
}

template <class G, bool FULL, bool INVD, bool SLIM, bool PB6, bool DW6 = false>
static int launch_bwd_pair_v(nf_ctx *ctx, const nf_flow_desc *desc, BwdAllArgs aa, float *stash, float *ybar, const float *lbar,
                             float lbar_const, float *slab, long slab_stride, int grid) {
  const size_t lds = BwdPairLds<G, PB6, DW6>::BYTES;
  NF_TRY((nf_lds_once<k_affine_bwd_pair<G, FULL, INVD, SLIM, PB6, DW6>>(ctx, lds)));
  if (PB6) {
    NF_TRY(b6t_refresh<G>(ctx, desc));
    aa.wimg_b6t = (const unsigned char *)ctx->wimg + b6t_offset_bytes<G>(desc);
  }
  ProfScope ps(ctx, INVD ? "affine_bwd_inv" : "affine_bwd");
  hipLaunchKernelGGL((k_affine_bwd_pair<G, FULL, INVD, SLIM, PB6, DW6>), dim3((unsigned)grid), dim3(512), lds, ctx->stream, aa, stash, ybar, lbar,
                     lbar_const, slab, slab_stride);
  return (int)hipGetLastError();
}
// NF_BWD_FP32=1: the A/B switch back to fp32-MFMA GEMMs in the pair kernel; NF_BWD_DW_FP32=1: only the consumer's dW GEMMs
template <class G, bool FULL, bool INVD>
static int launch_bwd_pair(nf_ctx *ctx, const nf_flow_desc *desc, const BwdAllArgs &aa, float *stash, float *ybar, const float *lbar,
                           float lbar_const, float *slab, long slab_stride, int grid) {
  static const bool fp32 = std::getenv("NF_BWD_FP32") != nullptr;
  if (stash_slim(G::SIZE)) return launch_bwd_pair_v<G, FULL, INVD, true, false>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid);
  static const bool dw_fp32 = std::getenv("NF_BWD_DW_FP32") != nullptr;
  if (fp32) return launch_bwd_pair_v<G, FULL, INVD, false, false>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid);
  return dw_fp32 ? launch_bwd_pair_v<G, FULL, INVD, false, true>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid)
                 : launch_bwd_pair_v<G, FULL, INVD, false, true, true>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid);
}

// reverse pass of all couplings from the stash nf_affine_chain_elbo(..., stash) left (same slab layout as
// nf_affine_bwd_all; ybar: cotangent of the flow output on entry, of the flow input on exit -- unless no_xbar: the caller,
// a training step, does not read it, and the two-wave kernel then leaves the last coupling's share of it unwritten)
int nf_affine_bwd_stashed(nf_ctx *ctx, const nf_flow_desc *desc, float *stash, float *ybar, const float *lbar, float lbar_const,
                          long N, float *slab, long slab_stride, int grid, bool inv_dir, bool no_xbar) {
  const int size = geo_size(desc);
  if (!size || !ctx->wimg || desc->n_hidden != 2 || !stash) return NF_ERR_UNSUPPORTED;
  BwdAllArgs aa;
  aa.wimg = (const float *)ctx->wimg;
  aa.wimg_b6t = nullptr;
  aa.trace = (long long *)ctx->trace;
  aa.d = desc->d;
  aa.ncoup = 2 * desc->nlayers;
  aa.N = N;
  aa.no_xbar = no_xbar ? 1 : 0;
  const bool h64 = size != NetGeo<1, 1, 1, 1>::SIZE;
  const bool full = desc->d == 64 && N % NF_TILE == 0;
  // hidden 33-64: the two-waves-per-tile kernel (both directions, ragged batches and d < 64 included)
  static const bool no_pair = std::getenv("NF_BWD_NO_PAIR") != nullptr;  // A/B switch: k_affine_bwd_stashed
  // (hidden <= 32 was measured with this kernel too: 226.9 against 227.8 us at d = 64, batch 65 536 -- no gain, not instantiated)
  if (h64 && !no_pair) {
    using GP = NetGeo<1, 2, 2, 1>;
    if (inv_dir)
      return full ? launch_bwd_pair<GP, true, true>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid)
                  : launch_bwd_pair<GP, false, true>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid);
    return full ? launch_bwd_pair<GP, true, false>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid)
                : launch_bwd_pair<GP, false, false>(ctx, desc, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid);
  }
  if (inv_dir) {  // forward-KL training: the stash of the inverse chain (nf_affine_chain(inverse, stash))
    if (h64)
      return full ? launch_bwd_stashed_v<NetGeo<1, 2, 2, 1>, true, true>(ctx, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid, desc)
                  : launch_bwd_stashed_v<NetGeo<1, 2, 2, 1>, false, true>(ctx, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid, desc);
    return launch_bwd_stashed_v<NetGeo<1, 1, 1, 1>, false, true>(ctx, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid, desc);
  }
  if (h64)
    return full ? launch_bwd_stashed_v<NetGeo<1, 2, 2, 1>, true>(ctx, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid, desc)
                : launch_bwd_stashed_v<NetGeo<1, 2, 2, 1>, false>(ctx, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid, desc);
  return full ? launch_bwd_stashed_v<NetGeo<1, 1, 1, 1>, true>(ctx, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid, desc)
              : launch_bwd_stashed_v<NetGeo<1, 1, 1, 1>, false>(ctx, aa, stash, ybar, lbar, lbar_const, slab, slab_stride, grid, desc);
}

// the two-hidden-layer kernels with their fused forward (draws + chain + target in one launch), stash and epilogue
bool nf_affine_fused_ok(const nf_flow_desc *desc) { return geo_size(desc) != 0; }
bool nf_affine_supported(const nf_flow_desc *desc) {
  if (nf_deep_geo_id(desc)) return true;
  if (desc->n_hidden != 2) return false;
  const int c = (desc->d + 1) / 2;  // larger of the two partitions
  const int mb = blocks32(c), h1b = blocks32(desc->hdims[0]), h2b = blocks32(desc->hdims[1]), cb = mb;
  (void)cb;
  return (mb == 1 && h1b == 1 && h2b == 1) || (mb == 1 && h1b == 2 && h2b == 2);
}
