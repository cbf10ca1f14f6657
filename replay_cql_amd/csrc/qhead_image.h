// The LDS image that the hand-scheduled Q-head kernels stream one operand through (qhead_de / de2 / de3 / fwd2 / fwd3 /
// argmax2 / topk2 / topk4 .hip), defined ONCE: where a staged 16-byte piece lands (img_off), where each lane reads it back
// (img_read_offsets), the LDS-DMA stager that fills it (ImgStager), and a compile-time check that the three agree.  Plus
// the small pieces those kernels share around it: exponential half-chunks, probability fragments, the AccVGPR product,
// owner-fragment loads.  The schedules (periods, gaps, ring turns) stay in the kernel files.
#pragma once
#include "qhead_internal.h"

typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(3))) f32x4 lds_f4;
typedef __attribute__((address_space(3))) bf16x8 lds_bf16x8;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

#define QDE_MAX_ITEMS 256  // items per group: 32 per wave, 4 or 8 waves per block
#ifndef QDE_VALU_HINT
#define QDE_VALU_HINT 32   // VALU instructions the scheduler is asked to place between the transposed reads and the 2nd chain
#endif

template <int D, int WAVES = 4>
struct DeCfg {
  static constexpr int ITEMS = 32 * WAVES;                   // items per group
  static constexpr int ROWB = 2 * D;
  static constexpr int KS = D / 16;
  static constexpr int FT = D / 32;
  static constexpr int TI = (D == 256) ? 32 : 64;            // states per stage
  static constexpr int TILES = TI / 32;
  static constexpr int STAGE_BYTES = TI * ROWB;              // 8 KiB (d=64) / 16 KiB
  static constexpr int LPS = STAGE_BYTES / 1024 / WAVES;     // LDS-DMA pieces (1 KiB) per wave per stage
  static constexpr int PPG = D / 64;                         // pieces per 8-row group
  static constexpr int RG_BYTES = 16 * D;                    // one 8-row group of the LDS image
  static constexpr int TILE_BYTES = 4 * RG_BYTES;            // 32 rows
  static constexpr int STRIP_BYTES = 256;                    // -lse*log2e of the stage's states: ONE copy per stage, loaded
                                                             // by wave (stage % WAVES)
  static constexpr int BUF_BYTES = STAGE_BYTES + STRIP_BYTES;
  static constexpr int PSTEP = WAVES * 1024;                 // source bytes between a wave's consecutive pieces
  static constexpr int NWAVES = WAVES;
  // piece WAVES i + wave lies in 8-row group (WAVES / PPG) i + wave / PPG: where WAVES / PPG is odd (d = 256 with 4 waves)
  // the group's parity, which enters the swizzle, alternates with i and a lane needs two source offsets
  static constexpr bool PAR_ALT = ((WAVES / PPG) & 1) != 0;
};

// ---- the image: 8-row x 32-column subtiles of 512 B --------------------------------------------------
// byte offset inside a stage of 16-byte chunk `ch` (8 bf16) of row `row`
template <class C>
constexpr int img_off(int row, int ch) {
  return C::RG_BYTES * (row >> 3) + 512 * (ch >> 2) + 64 * (row & 7) + 16 * ((ch & 3) ^ ((row >> 2) & 3));
}

// Per-lane read offsets inside a buffer (r = lane & 31, h = lane >> 5).
//  oa0 / oa1: A operand of a score chain, row r of a 32-row tile, chunk 2 s + h -> oa<s & 1> + 512 (s >> 1) [+ TILE_BYTES it]
//  ot0 / ot1: ds_read_tr16_b64, lane 4 q + p of 16-lane group (g1, h): row 16 s2 + 8 jj + 4 h + q, chunk 4 ft + 2 g1 + (p >> 1),
//             half (p & 1) of it -> ot<jj> + RG_BYTES (2 s2 + jj) + 512 ft
//  os:        the strip's four floats of accumulator quarter q (rows 8 q + 4 h ..) -> os + 128 it + 32 q
struct ImgRead {
  int oa0, oa1, ot0, ot1, os;
};
template <class C>
constexpr ImgRead img_read_offsets(int lane) {
  const int r = lane & 31, h = lane >> 5;
  const int g1 = (lane >> 4) & 1, q = (lane & 15) >> 2, p = lane & 3;
  return {C::RG_BYTES * (r >> 3) + 64 * (r & 7) + 16 * ((0 + h) ^ ((r >> 2) & 3)),
          C::RG_BYTES * (r >> 3) + 64 * (r & 7) + 16 * ((2 + h) ^ ((r >> 2) & 3)),
          64 * (4 * h + q) + 16 * ((2 * g1 + (p >> 1)) ^ ((0 + h) & 3)) + 8 * (p & 1),
          64 * (4 * h + q) + 16 * ((2 * g1 + (p >> 1)) ^ ((2 + h) & 3)) + 8 * (p & 1),
          C::STAGE_BYTES + 16 * h};
}

// Staging: piece pc = WAVES i + wave of a stage is 1 KiB of the image, [1024 pc, 1024 pc + 1024); lane l fills its bytes
// [16 l, 16 l + 16): subtile l >> 5, row (l >> 2) & 7, slot l & 3 = (chunk & 3) ^ ((row >> 2) & 3).  This is the lane's
// source offset inside the stage for piece i = 0 (par = parity of i where C::PAR_ALT); piece i adds C::PSTEP * i.
template <class C>
constexpr uint32_t img_stage_voff(int lane, int wave, int par) {
  const int sub = lane >> 5, r7 = (lane >> 2) & 7, slot = lane & 3;
  const int rg0 = wave / C::PPG, hc = wave % C::PPG;
  const int rg1 = (C::PAR_ALT ? (rg0 + par) : rg0) & 1;
  const int q2 = (r7 >> 2) | (rg1 << 1);
  return (uint32_t)((rg0 * 8 + r7) * C::ROWB + (8 * hc + 4 * sub + (slot ^ q2)) * 16);
}

// The one invariant these kernels rest on: staging and reads agree on img_off.
template <class C>
constexpr bool img_geometry_ok() {
  for (int lane = 0; lane < 64; ++lane) {
    const ImgRead o = img_read_offsets<C>(lane);
    const int r = lane & 31, h = lane >> 5, g1 = (lane >> 4) & 1, q = (lane & 15) >> 2, p = lane & 3;
    for (int it = 0; it < C::TILES; ++it) {
      for (int s = 0; s < C::KS; ++s)
        if (((s & 1) ? o.oa1 : o.oa0) + 512 * (s >> 1) + C::TILE_BYTES * it != img_off<C>(32 * it + r, 2 * s + h)) return false;
      for (int ft = 0; ft < C::FT; ++ft)
        for (int s2 = 0; s2 < 2; ++s2)
          for (int jj = 0; jj < 2; ++jj)
            if ((jj ? o.ot1 : o.ot0) + C::RG_BYTES * (2 * s2 + jj) + 512 * ft + C::TILE_BYTES * it !=
                img_off<C>(32 * it + 16 * s2 + 8 * jj + 4 * h + q, 4 * ft + 2 * g1 + (p >> 1)) + 8 * (p & 1))
              return false;
      for (int e = 0; e < 16; ++e)      // strip: one float per row, element e of the accumulator = row 8 (e >> 2) + 4 h + (e & 3)
        if (o.os + 128 * it + 32 * (e >> 2) + 4 * (e & 3) != C::STAGE_BYTES + 4 * (32 * it + 8 * (e >> 2) + 4 * h + (e & 3)))
          return false;
    }
    for (int wave = 0; wave < C::NWAVES; ++wave)
      for (int i = 0; i < C::LPS; ++i) {
        const int src = (int)img_stage_voff<C>(lane, wave, i & 1) + C::PSTEP * i;      // byte of the stage's row-major source
        if ((C::NWAVES * i + wave) * 1024 + 16 * lane != img_off<C>(src / C::ROWB, (src % C::ROWB) / 16)) return false;
      }
  }
  return C::LPS * C::NWAVES * 1024 == C::STAGE_BYTES;
}
static_assert(img_geometry_ok<DeCfg<64, 4>>() && img_geometry_ok<DeCfg<128, 4>>() && img_geometry_ok<DeCfg<256, 4>>() &&
              img_geometry_ok<DeCfg<64, 8>>() && img_geometry_ok<DeCfg<128, 8>>() && img_geometry_ok<DeCfg<256, 8>>(),
              "LDS image: staged pieces and per-lane reads must agree on img_off");

struct QDeArgs {
  const uint16_t* H_b;      // [n_states x D] streamed
  const float* nlse2;       // [n_states]  -lse * log2e
  int64_t n_states;
  const uint16_t* E_b;      // [n_items x D] owner rows (already offset to the first item of this call)
  const float* bias;        // [n_items]
  int64_t n_items;
  float* out;               // [n_items x D]
  float* out_cs;            // [n_items]
  float scale;
  int accumulate;           // out / out_cs hold the one-hot part already
  float* slab;              // [grid][ITEMS x D]   pieces that do not hold stage 0 of their group
  float* slab_cs;           // [grid][ITEMS]
  int32_t G, T;             // item groups, stages per group
  unsigned long long* stamps;   // diagnostic (CQL_QDE_STAMPS=1): per block {shader-clock ticks, 100 MHz ticks} of its run; else NULL
};

// clock stamps of a diagnostic run: written to a buffer no other code reads (never part of an output)
__device__ __forceinline__ void qde_stamp(unsigned long long& tk, unsigned long long& rt) {
  tk = __builtin_amdgcn_s_memtime();
  rt = __builtin_amdgcn_s_memrealtime();
}

__device__ __forceinline__ uint32_t lds_addr_of(const void* p) { return (uint32_t)(uintptr_t)(lds_void_t*)p; }

// LDS-DMA: 64 lanes x 16 B -> 1 KiB at LDS byte `lds_dst` (wave-uniform), source = descriptor base + voff (per lane) + soff
__device__ __forceinline__ void bdma16(uint32_t voff, __amdgpu_buffer_rsrc_t rsrc, uint32_t soff, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void bdma4(uint32_t voff, __amdgpu_buffer_rsrc_t rsrc, uint32_t soff, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_dst) : "memory");
}

template <int N>
__device__ __forceinline__ void de_wait_vmcnt() {
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else static_assert(N < 0, "add the vmcnt literal");
}

// buffer descriptor over `bytes` bytes at `ptr`: raw buffer, out-of-range loads return 0 (the kernels rely on that past the
// end of a table)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* ptr, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)ptr, 0, (int)bytes, 0x00020000);
}

// LDS-DMA of one stage (rows + strip) into ring buffer `buf` (BUF bytes apart).  `stage` is the kernel's own stage index --
// the strip is loaded by wave (stage % WAVES) -- and stage0 + stage the stage's index in the source tables.  A kernel's
// extra streams (seen words of the top-k kernels) stay in the kernel.
template <class C, int BUF = C::BUF_BYTES>
struct ImgStager {
  uint32_t voff[C::PAR_ALT ? 2 : 1];
  uint32_t voff_strip;
  uint32_t smem_base;
  uint32_t stage0;
  int wave;
  __amdgpu_buffer_rsrc_t rs_rows, rs_strip;
  __device__ __forceinline__ ImgStager(int lane, int wave_, uint32_t smem_base_, uint32_t stage0_, __amdgpu_buffer_rsrc_t rows,
                                       __amdgpu_buffer_rsrc_t strip_)
      : voff_strip((uint32_t)lane * 4), smem_base(smem_base_), stage0(stage0_), wave(wave_), rs_rows(rows), rs_strip(strip_) {
#pragma unroll
    for (int par = 0; par < (C::PAR_ALT ? 2 : 1); ++par) voff[par] = img_stage_voff<C>(lane, wave_, par);
  }
  __device__ __forceinline__ uint32_t buf_lds(int buf) const { return __builtin_amdgcn_readfirstlane(smem_base + buf * BUF); }
  __device__ __forceinline__ void piece(int stage, int buf, int i) const {
    const uint32_t bufp = buf_lds(buf);
    const uint32_t gs = stage0 + (uint32_t)stage;
    bdma16(voff[C::PAR_ALT ? (i & 1) : 0], rs_rows, gs * C::STAGE_BYTES + C::PSTEP * i, bufp + (C::NWAVES * i + wave) * 1024);
  }
  __device__ __forceinline__ void strip(int stage, int buf) const {
    const uint32_t bufp = buf_lds(buf);
    const uint32_t gs = stage0 + (uint32_t)stage;
    if (wave == (stage & (C::NWAVES - 1))) bdma4(voff_strip, rs_strip, gs * (C::TI * 4), bufp + C::STAGE_BYTES);
  }
  __device__ __forceinline__ void all(int stage, int buf) const {
#pragma unroll
    for (int i = 0; i < C::LPS; ++i) piece(stage, buf, i);
    strip(stage, buf);
  }
};

// Rows past the end of the streamed table (last stage of the last slice) read as 0 (buffer bounds); a strip value of -inf
// makes their scores -inf and their probabilities exactly 0.  `valid` = rows of the stage that exist; block-uniform; called
// between a barrier behind the stage's landing and the first read of its strip.
template <class C, int BUF = C::BUF_BYTES>
__device__ __forceinline__ void img_patch_strip(lds_u8* smem, int buf, const int64_t valid, const int& lane, const int& wave) {
  if (valid < C::TI) {
    if (wave == 0 && lane < C::TI && lane >= valid)
      *(__attribute__((address_space(3))) float*)(smem + buf * BUF + C::STAGE_BYTES + lane * 4) = NEG_INF_F;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();
  }
}

// ---- pieces of the pipelined periods ---------------------------------------------------------------------------------
// One "chunk" of the exponentials (two probabilities) in two halves, one per MFMA gap; ht0 / ht1 travel from a() to b().
// Volatile asm: hipcc would otherwise regroup them (sinks the column sums to the end of the stage as v_pk_add_f32 and keeps
// every exponential alive).  b() reads a v_exp result one instruction later at the earliest (gfx950: one wait state behind
// a transcendental).  a(): P = exp2(acc * log2e + b), the addends of elements 2 k and 2 k + 1.
struct QExpPair {
  float ht0 = 0.f, ht1 = 0.f;
  __device__ __forceinline__ void a(const f32x16& acc, int k, float b0, float b1) {
    asm volatile(
        "v_fmamk_f32 %0, %2, 0x3fb8aa3b, %4\n\t"
        "v_fmamk_f32 %1, %3, 0x3fb8aa3b, %5\n\t"
        "v_exp_f32 %0, %0"
        : "=&v"(ht0), "=&v"(ht1)
        : "v"(acc[2 * k]), "v"(acc[2 * k + 1]), "v"(b0), "v"(b1));
  }
  __device__ __forceinline__ void b(uint32_t& w, float& csum) {
    asm volatile(
        "v_exp_f32 %1, %1\n\t"
        "v_add_f32 %3, %3, %0\n\t"
        "v_add_f32 %3, %3, %1\n\t"
        "v_cvt_pk_bf16_f32 %2, %0, %1"
        : "+v"(ht0), "+v"(ht1), "=&v"(w), "+v"(csum));
  }
};
// probability fragment s2 (B operand of the second product) from the eight packed words of a tile
__device__ __forceinline__ bf16x8 q_frag(const uint32_t (&pw)[8], int s2) {
  u32x4 v = {pw[4 * s2 + 0], pw[4 * s2 + 1], pw[4 * s2 + 2], pw[4 * s2 + 3]};
  return __builtin_bit_cast(bf16x8, v);
}
// Y += A . B with the accumulator in AccVGPRs, as inline asm: the builtin form of these translation units
// (-amdgpu-mfma-vgpr-form, which the score chains need: the VALU reads their results) would put the 128 accumulator
// registers of Y into the VGPR half too, and the rest of the kernel then no longer fits there -- hipcc parks owner
// fragments in AccVGPRs and copies them back in front of every product.  A = transposed fragment (VGPRs: where hipcc lets
// the ds_read_tr land), B = probability fragment (VGPRs).  The leading s_nop covers "VALU wrote B just before" (the
// hazard recogniser does not look into asm); products on the same accumulator are four products apart.
__device__ __forceinline__ void q_mfma_y_acc(f32x16& y, const bf16x8& a_frag, const bf16x8& b_frag) {
  const u32x4 av = __builtin_bit_cast(u32x4, a_frag), bv = __builtin_bit_cast(u32x4, b_frag);
  asm volatile("s_nop 1\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(y) : "v"(av), "v"(bv));
}
// MFMA B fragments of owner row `row` (clamped to the table's last row; h = lane >> 5)
template <int D>
__device__ __forceinline__ void load_owner_frags(const uint16_t* base, int64_t row, int64_t n_rows, int h, bf16x8 (&rf)[D / 16]) {
  if (row >= n_rows) row = n_rows - 1;
#pragma unroll
  for (int s = 0; s < D / 16; ++s) rf[s] = *reinterpret_cast<const bf16x8*>(base + row * D + 16 * s + 8 * h);
}
// Ordinary loads (owner fragments, bias) must be retired -- in hipcc's own bookkeeping too -- before the next LDS-DMA is
// issued: its counted waits assume that nothing younger than its loads is in flight (cdna_hip_programming.md 5, trap
// (b)).  The builtin is a wait the compiler models (vmcnt(0) only: 0x0F70); an empty asm with "+v" operands would do as
// well but pins the fragments to the VGPR half, and the MFMA operands then get copied to AGPRs in every loop trip.
__device__ __forceinline__ void owner_fence() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}


// End of a piece (qde_pieces.h), one wave's 32 items: y = the FT accumulators of gradient row `row` (lane's item) and its
// slab twin `srow` (qde_slab_row of this block), cs = this lane half's column sum.  The piece that holds stage 0 goes to
// the gradient, scaled (written, or added to what is there); any other unscaled to the slab (rows past n_items: harmless,
// not read).  No caller of cql_qde_launch passes accumulate != 0 today: that branch, here and in qde_kernel's own store,
// is reached by no entry point and covered by no test.
template <int D>
__device__ __forceinline__ void qde_store_group(const QDeArgs& a, bool first, int64_t row, int64_t srow, int h,
                                                const f32x16 (&y)[D / 32], float cs) {
  const float csum = cs + __shfl_xor(cs, 32);
  if (first) {
    if (row < a.n_items) {
      float* dst = a.out + row * D;
#pragma unroll
      for (int ft = 0; ft < D / 32; ++ft)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float4* pd = reinterpret_cast<float4*>(dst + ft * 32 + 8 * q + 4 * h);
          float4 o;
          if (a.accumulate) {
            const float4 old = *pd;
            o = make_float4(qde_axpy(old.x, a.scale, y[ft][4 * q + 0]), qde_axpy(old.y, a.scale, y[ft][4 * q + 1]),
                            qde_axpy(old.z, a.scale, y[ft][4 * q + 2]), qde_axpy(old.w, a.scale, y[ft][4 * q + 3]));
          } else {
            o = make_float4(a.scale * y[ft][4 * q + 0], a.scale * y[ft][4 * q + 1], a.scale * y[ft][4 * q + 2],
                            a.scale * y[ft][4 * q + 3]);
          }
          *pd = o;
        }
      if (h == 0) a.out_cs[row] = a.accumulate ? qde_axpy(a.out_cs[row], a.scale, csum) : a.scale * csum;
    }
  } else {
    float* dst = a.slab + srow * D;
#pragma unroll
    for (int ft = 0; ft < D / 32; ++ft)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<float4*>(dst + ft * 32 + 8 * q + 4 * h) =
            make_float4(y[ft][4 * q + 0], y[ft][4 * q + 1], y[ft][4 * q + 2], y[ft][4 * q + 3]);
    if (h == 0) a.slab_cs[srow] = csum;
  }
}

// qhead_de2.hip: 64 items per wave, one wave per SIMD (d = 128).  `a.nlse2` holds -lse in NATURAL units there.
int cql_qde2_run(const QDeArgs& a, int d, int grid, hipStream_t s);
// qhead_de3.hip: 32 items per wave, one wave per SIMD, in-wave pipeline (d = 256).  -lse in NATURAL units as for qde2.
int cql_qde3_run(const QDeArgs& a, int d, int grid, hipStream_t s);
