// Host-only check of the fused planar / radial / mean-field ELBO step's routing predicate and workspace layout
// (step_fusable_simple, SimpleStepBufs in nf_api.hip).  Built by tests/test_simple_step_cpu.py the way tests/test_sanitizers.py
// builds nf_api_host_check.hip: every translation unit's host side under -fsanitize=address,undefined, a hand-made nf_ctx, no
// device -- the carving code only does pointer arithmetic on a fake arena address that is never dereferenced.
// This TU includes nf_api.hip to reach its file-local functions.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../normalizingflows.jl_amd/csrc/nf_api.hip"

static int fails = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "CHECK failed at line %d: %s\n", __LINE__, #cond);    \
      ++fails;                                                                   \
    }                                                                            \
  } while (0)

static nf_flow_desc mk(int kind, int dtype, int d, int nl) {
  nf_flow_desc g;
  std::memset(&g, 0, sizeof g);
  g.kind = kind;
  g.dtype = dtype;
  g.d = d;
  g.nlayers = nl;
  return g;
}

int main() {
  nf_ctx ctx;  // hand-made: no device, no stream, nothing is launched
  ctx.num_cu = 256;
  const nf_flow_desc flows[] = {mk(NF_KIND_PLANAR, NF_DTYPE_F32, 64, 10), mk(NF_KIND_PLANAR, NF_DTYPE_F64, 2, 10),
                                mk(NF_KIND_RADIAL, NF_DTYPE_F32, 5, 10), mk(NF_KIND_MEANFIELD, NF_DTYPE_F64, 4, 1),
                                mk(NF_KIND_PLANAR, NF_DTYPE_F32, 200, 30)};
  const bool fused[] = {true, true, true, true, false};
  nf_target banana;
  std::memset(&banana, 0, sizeof banana);
  banana.kind = NF_TARGET_BANANA;
  banana.s0 = 1.0;
  banana.s1 = 10.0;
  nf_target warped = banana;  // two-dimensional: its check fails at any other d
  warped.kind = NF_TARGET_WARPED;
  warped.s1 = 0.12;
  int dummy_comm = 0;
  const long Ns[] = {1, 15, 16, 17, 1000, 65536};
  for (long budget : {-1L, 0L, 3L << 20}) {
    ctx.stash_budget = budget;
    for (int f = 0; f < 5; ++f) {
      const nf_flow_desc &g = flows[f];
      CHECK(check_desc(&g) == NF_OK);
      // the predicate: sizing form, with a target that passes its check, with one that fails it, under a communicator
      CHECK(step_fusable_simple(&ctx, &g, nullptr, true) == fused[f]);
      CHECK(step_fusable_simple(&ctx, &g, &banana) == fused[f]);
      CHECK(step_fusable_simple(&ctx, &g, &warped) == (fused[f] && g.d == 2));
      ctx.comm = &dummy_comm;
      CHECK(!step_fusable_simple(&ctx, &g, &banana));
      CHECK(step_fusable_simple(&ctx, &g, nullptr, true) == fused[f]);  // sized whatever the communicator
      ctx.comm = nullptr;
      nf_base base;
      base.kind = NF_BASE_DIAG;
      base.mu = base.scale = &dummy_comm;
      base.logdet = 0;
      nf_flow_desc gb = g;
      gb.base = &base;
      CHECK(!step_fusable_simple(&ctx, &gb, &banana));
      if (!fused[f]) continue;
      for (long N : Ns) {
        const size_t need = layout_bytes<SimpleStepBufs>(&ctx, &g, N);
        const size_t tail = ws_tail_bytes(&ctx, &g, N);
        const int64_t total = nf_workspace_bytes(&ctx, &g, N);
        CHECK(need % 256 == 0);
        CHECK(need + tail <= (size_t)total);
        CHECK(need <= ws_need_bound(&ctx, &g, N));
        CHECK(need <= layout_bytes<VgBufs>(&ctx, &g, N));  // no larger than the split form's layout
        // the carve inside an arena of exactly `total` bytes: aligned, disjoint, in front of the tails
        char *fake = (char *)(uintptr_t)0x7f0000000000ull;  // never dereferenced
        ctx.arena = fake;
        ctx.arena_bytes = (size_t)total;
        ctx.arena_tail = ctx.arena_front = 0;
        ctx.ws = ctx.wimg = ctx.gbuf = nullptr;
        ctx.ws_bytes = ctx.wimg_bytes = ctx.gbuf_bytes = 0;
        SimpleStepBufs b;
        CHECK(ws_carve(&ctx, &b, &g, N) == NF_OK);
        void *gb = nullptr;  // nf_elbo_step's [grad ; loss ; norm] buffer: a tail carve (gbuf_reserve, without its memset)
        const size_t gneed = gbuf_need(nf_param_count(&g), esize(g.dtype));
        CHECK(arena_tail_take(&ctx, gneed, &gb) == NF_OK);
        const size_t nb_part = (size_t)elbo_npartial(&ctx, &g, N) * 8, nb_slab = nf_simple_step_ws_bytes(&ctx, &g, N);
        const size_t nb_gpart = (size_t)b.eblocks * 8;
        CHECK(b.eblocks == (g.kind == NF_KIND_MEANFIELD ? 2 : g.nlayers));
        // the step launch writes one loss partial per workgroup: at most one per 16 samples, capped by the resident-block bound
        const long nwg = (N + 15) / 16 < nf_simple_elbo_max_partials(&ctx) ? (N + 15) / 16 : nf_simple_elbo_max_partials(&ctx);
        CHECK(nwg <= elbo_npartial(&ctx, &g, N));
        char *p[3] = {(char *)b.partial, b.slabs, (char *)b.gpart};
        const size_t len[3] = {nb_part, nb_slab, nb_gpart};
        for (int i = 0; i < 3; ++i) {
          CHECK(((uintptr_t)p[i] & 255) == 0);
          CHECK(p[i] >= fake && p[i] + len[i] <= fake + need);
          for (int j = i + 1; j < 3; ++j) CHECK(p[i] + len[i] <= p[j] || p[j] + len[j] <= p[i]);
        }
        CHECK((char *)gb >= fake + need && (char *)gb + gneed <= fake + total);
        ctx.arena = nullptr;
        ctx.ws = ctx.wimg = ctx.gbuf = nullptr;
        ctx.ws_bytes = ctx.wimg_bytes = ctx.gbuf_bytes = 0;
      }
    }
  }
  if (fails) {
    std::fprintf(stderr, "%d check(s) failed\n", fails);
    return 1;
  }
  std::printf("nf_simple_step host check: ok\n");
  return 0;
}
