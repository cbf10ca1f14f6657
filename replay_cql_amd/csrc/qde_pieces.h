// The cut of the item-side backward (dE_out), stated once.  Normative for qde_kernel / qde2_kernel / qde3_kernel (the
// writers), qde_fixup_kernel and adam_fix4 (the readers), cql_qde_launch (the plan) and tests/helpers.qde_geometry (held
// to this file by tests/asan/host_driver.cpp).
//
// W = G T stage-units (G item groups x T stages of states) are dealt to nblk persistent blocks in contiguous, equal
// ranges: block p owns [start(p), start(p + 1)), start(p) = floor(p W / nblk).  A group that straddles ranges is summed in
// pieces: the piece that holds stage 0 goes to the gradient, scaled; every other piece goes UNSCALED to slab row
// p items + row of the block p that formed it (a block starts at most one such piece: its first); a reader adds
// scale * slab to the gradient, piece by piece in block order, as a product and then a sum (qde_axpy).
//
// Integer code and one float expression; plain C++ and HIP device code alike, no HIP header needed.
#pragma once
#include <stdint.h>

#ifdef __HIP__
#define QDE_HD __attribute__((host)) __attribute__((device)) __attribute__((always_inline)) inline
#else
#define QDE_HD inline
#endif

struct QdePieces {
  int32_t G, T, nblk;      // item groups, stages per group, blocks of the long kernel

  QDE_HD int64_t W() const { return (int64_t)G * T; }
  QDE_HD int64_t start(int64_t p) const { return p * W() / nblk; }
  QDE_HD bool empty(int64_t p) const { return start(p + 1) == start(p); }      // nblk > W: such a block writes nothing

  // a block's prologue: its range (nst stage-units from u0; nst = 0: nothing to do), then the group and the stage
  // inside the group of a unit -- of u0, where the block begins
  struct Range { int64_t u0; int nst; };
  QDE_HD Range range(int64_t p) const {
    const int64_t u0 = start(p);
    return {u0, (int)(start(p + 1) - u0)};
  }
  struct Unit { int g, t; };
  QDE_HD Unit unit(int64_t u) const {
    const int g = (int)(u / T);
    return {g, (int)(u - (int64_t)g * T)};
  }

  // does some block start inside a group (is there a slab piece at all)?
  QDE_HD bool any_cut() const {
    for (int64_t p = 1; p < nblk; ++p)
      if (start(p) % T != 0) return true;
    return false;
  }
};

// The slab pieces of group g, in block order, as a statement head: `QDE_FOR_SLAB_PIECES(I, L, pc, g, p) { ... }` runs its
// body for every block p whose first piece is a slab piece of g -- start(p) strictly inside (g T, (g + 1) T) and the
// range not empty.  I = index type, L = the type p W is formed in: (uint32_t, uint64_t) where W (nblk + 1) < 2^31 is
// known, else (int64_t, int64_t).  A macro, not a callable: through a callable hipcc builds adam_ema_fix_kernel's loop
// differently (profiles/qde_pieces_ab.md).
#define QDE_FOR_SLAB_PIECES(I, L, pc, g, p)                                                                  \
  for (I w_ = (I)(pc).G * (I)(pc).T, nb_ = (I)(pc).nblk, lo_ = (g) * (I)(pc).T, hi_ = lo_ + (I)(pc).T,       \
         p = ((lo_ + 1) * nb_ + w_ - 1) / w_;                                                                \
       p < nb_; ++p)                                                                                         \
    if (const I u0_ = (I)((L)p * w_ / nb_); u0_ >= hi_) break;                                               \
    else if (u0_ <= lo_ || (I)(((L)p + 1) * w_ / nb_) == u0_) continue;                                      \
    else

// slab row of in-group row `row` of block p's piece; the same index addresses the piece's column sums
QDE_HD int64_t qde_slab_row(int64_t p, int items, int64_t row) { return p * items + row; }

// w + scale * u as a product and a sum, never an fma, whatever the translation unit's contraction mode: every path to
// the gradient (the long kernels' accumulate, the fix-up launch, the fix inside the item-side Adam) gives the same bits
QDE_HD float qde_axpy(float w, float scale, float u) {
#pragma clang fp contract(off)
  const float su = scale * u;
  return w + su;
}

// what the readers need of a launch of the long kernel
struct QdeSlab {
  const float* slab;       // [nblk][items x D]
  const float* slab_cs;    // [nblk][items]
  QdePieces pc;
  int32_t items, D;
  float scale;
  int64_t n_items;
  QDE_HD const float* row(int64_t p, int64_t row) const { return slab + qde_slab_row(p, items, row) * D; }
  QDE_HD const float* cs(int64_t p, int64_t row) const { return slab_cs + qde_slab_row(p, items, row); }
};

// Deferred sum of the slab pieces.  The single-rank step driver skips the fix-up launch: the Adam launch that consumes
// g_E_out / g_b_out right behind the long kernel adds the same slabs, in the same order, while it reads the gradient
// (cql_adam_ema_fix, adam_math.h) -- one launch and one read-modify-write of the cut rows less on the step's critical path.
struct CqlAdamFix {
  int valid;                // 0: nothing deferred (the gradient is complete)
  QdeSlab s;
  int64_t rows_off, cs_off; // element offsets of g_E_out / g_b_out inside the updated range
};

// ---- which kernel, which groups and stages, how many blocks ---------------------------------------------------------
enum { QDE_FORM_GENERIC = 1, QDE_FORM_2 = 2, QDE_FORM_3 = 3 };
// form 2 (qhead_de2.hip: d = 128, whole stages of 64 states), form 3 (qhead_de3.hip: d = 256, whole stages of 32), else
// qde_kernel<d> (qhead_de.hip).  Forms 2 and 3 have the groups, stages and grid of the generic form they replace.
QDE_HD int qde_form(int d, int64_t batch) {
  return (d == 128 && batch % 64 == 0) ? QDE_FORM_2 : (d == 256 && batch % 32 == 0) ? QDE_FORM_3 : QDE_FORM_GENERIC;
}
// items per group: 32 per wave, 8 waves -- 4 at d = 256, where the register budget forbids two waves per SIMD
constexpr int qde_items(int d) { return d == 256 ? 128 : 256; }
constexpr int qde_stage_states(int d) { return d == 256 ? 32 : 64; }

struct QdePlan {
  int form;
  int32_t items, ti;       // items per group, states per stage
  QdePieces pc;            // G, T and the grid: one persistent block per CU, fewer when there are fewer stage-units
};
// n_cu: the device's CU count; anything outside 1 .. 256 counts as 256
QDE_HD QdePlan qde_plan(int64_t batch, int64_t n_items, int d, int n_cu) {
  if (n_cu <= 0 || n_cu > 256) n_cu = 256;
  QdePlan pl = {qde_form(d, batch), qde_items(d), qde_stage_states(d), {}};
  pl.pc.G = (int32_t)((n_items + pl.items - 1) / pl.items);
  pl.pc.T = (int32_t)((batch + pl.ti - 1) / pl.ti);
  pl.pc.nblk = (int32_t)(pl.pc.W() < n_cu ? pl.pc.W() : n_cu);
  return pl;
}
