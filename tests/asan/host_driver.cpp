// AddressSanitizer driver of the HOST side of libcqlrec ("-fsanitize=address host build of the C++ op layer").
// Linked against the host-only, ASan-instrumented build of the library (replay_cql_amd/build.py::build_asan: hipcc
// --cuda-host-only -fsanitize=address -- GPU ASan is not available on the pool, and nothing here launches a kernel).
// It walks every entry point's argument validation and error reporting (CQL_REQUIRE -> cql_set_error: formatted into
// a thread-local buffer), the size / split / layout arithmetic, and the workspace-size functions over a grid of
// shapes, exactly as a caller without a GPU can reach them.  Exit code 0 and no ASan report = pass.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "../../include/cqlrec.h"
#include "../../replay_cql_amd/csrc/qde_pieces.h"

static int fails = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "host_driver: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                               \
    }                                                                        \
  } while (0)

static void layouts() {
  const int64_t ns[] = {1, 4, 63, 64, 65, 257, 3883, 10007, 100000, 1000000};
  const int32_t ds[] = {64, 128, 256};
  for (int64_t n : ns)
    for (int32_t d : ds) {
      cqlrec_layout l;
      memset(&l, 0xAB, sizeof l);
      EXPECT(cqlrec_layout_make(n, d, &l) == CQLREC_OK);
      EXPECT(l.n_items == n && l.d == d && l.off_E_in == 0);
      EXPECT(l.off_E_out >= (n + 1) * d && l.off_E_out % CQLREC_SEG_ALIGN == 0);
      EXPECT(l.off_b_out >= l.off_E_out + n * d && l.off_W1 >= l.off_b_out + n && l.total % CQLREC_SEG_ALIGN == 0);
      EXPECT(l.total >= l.off_b2 + d);
    }
  cqlrec_layout l;
  EXPECT(cqlrec_layout_make(0, 128, &l) != CQLREC_OK);
  EXPECT(cqlrec_layout_make(100, 100, &l) != CQLREC_OK);
  EXPECT(cqlrec_layout_make(100, 128, nullptr) != CQLREC_OK);
  EXPECT(strlen(cqlrec_last_error()) > 0);
}

static void workspace_sizes() {
  const int64_t users[] = {1, 63, 256, 257, 4000, 62500, 65536};
  const int64_t items[] = {1, 31, 64, 1000, 3883, 10007, 100000, 1000000};
  const int32_t ds[] = {64, 128, 256};
  for (int64_t u : users)
    for (int64_t n : items)
      for (int32_t d : ds) {
        const int64_t a = cqlrec_topk_ws_bytes(u, n, d, 10);
        EXPECT(a > 0 && a % 256 == 0);
        EXPECT(cqlrec_topk_ws_bytes(u, n, d, 2048) >= 0);
        if (u <= 4096) {
          EXPECT(cqlrec_qhead_ws_bytes(u, n, d) > 0);
          EXPECT(cqlrec_qhead_bwd_ws_bytes(u, n, d) > 0);
          EXPECT(cqlrec_qhead_fused_ws_bytes(u, n, d) > 0);
          EXPECT(cqlrec_train_ws_bytes((int32_t)u, n, d, 50) > 0);
          EXPECT(cqlrec_gather_pool_bwd_ws_bytes(u, 50, d) > 0);
          EXPECT(cqlrec_encoder_bwd_ws_bytes(u, d) > 0);
        }
      }
  EXPECT(cqlrec_build_csr_ws_bytes(0) >= 0);
  EXPECT(cqlrec_build_csr_ws_bytes(1000003) > 0);
  EXPECT(cqlrec_eval_topk_ws_bytes(4096, 3) >= 0);
}

// every call below must be REFUSED by the argument checks in front of any launch (no GPU is needed, none is touched)
static void refused_calls() {
  std::vector<uint16_t> h16(64 * 128);
  std::vector<float> f32(4096);
  std::vector<int32_t> i32(4096);
  std::vector<int64_t> i64(4096);
  std::vector<unsigned char> ws(1 << 16);
  void* p = ws.data();
  EXPECT(cqlrec_score_topk(nullptr, 8, h16.data(), f32.data(), 64, 128, nullptr, nullptr, nullptr, nullptr, 4, p, 1 << 16,
                           i32.data(), f32.data(), i32.data(), nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_score_topk(h16.data(), 8, h16.data(), f32.data(), 64, 100, nullptr, nullptr, nullptr, nullptr, 4, p, 1 << 16,
                           i32.data(), f32.data(), i32.data(), nullptr) == CQLREC_ERR_INVALID);      // d unsupported
  EXPECT(cqlrec_score_topk(h16.data(), 8, h16.data(), f32.data(), 64, 128, nullptr, nullptr, nullptr, nullptr, 0, p, 1 << 16,
                           i32.data(), f32.data(), i32.data(), nullptr) == CQLREC_ERR_INVALID);      // k out of range
  EXPECT(cqlrec_score_topk(h16.data(), 8, h16.data(), f32.data(), 64, 128, nullptr, i64.data(), nullptr, nullptr, 4, p,
                           1 << 16, i32.data(), f32.data(), i32.data(), nullptr) == CQLREC_ERR_INVALID);   // seen_items NULL
  EXPECT(cqlrec_score_topk(h16.data(), 4000, h16.data(), f32.data(), 5000, 128, nullptr, nullptr, nullptr, nullptr, 4, p, 16,
                           i32.data(), f32.data(), i32.data(), nullptr) == CQLREC_ERR_INVALID);      // workspace too small
  EXPECT(cqlrec_score_topk_phase(h16.data(), 8, h16.data(), f32.data(), 64, 128, nullptr, nullptr, nullptr, nullptr, 4, p,
                                 1 << 16, i32.data(), f32.data(), i32.data(), 77, nullptr) == CQLREC_ERR_INVALID);
  EXPECT(strstr(cqlrec_last_error(), "phase") != nullptr);
  EXPECT(cqlrec_adam_ema(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 64, 1e-3f, 1.f, 0.9f, 0.999f, 1e-8f,
                         0.005f, 1, nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_adam_ema(f32.data(), f32.data(), f32.data(), f32.data(), f32.data(), h16.data(), h16.data(), 6, 1e-3f, 1.f,
                         0.9f, 0.999f, 1e-8f, 0.005f, 1, nullptr) == CQLREC_ERR_INVALID);             // n % 4 != 0
  EXPECT(cqlrec_qhead_fwd(nullptr, 8, h16.data(), f32.data(), 64, 128, 0, p, 1 << 16, f32.data(), nullptr, nullptr,
                          nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_gather_dot(nullptr, h16.data(), f32.data(), i32.data(), 8, 128, f32.data(), nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_linear_bf16(nullptr, h16.data(), f32.data(), 8, 128, 1, nullptr, h16.data(), nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_gather_pool_fwd(nullptr, i64.data(), i32.data(), i32.data(), nullptr, 0, 8, 50, 128, f32.data(), nullptr,
                                nullptr, nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_build_csr(nullptr, nullptr, nullptr, nullptr, 10, 4, p, 1 << 16, i64.data(), i32.data(), f32.data(),
                          nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_train_steps(nullptr, 0, 1, nullptr, nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_train_views_get(nullptr, 0, nullptr) == CQLREC_ERR_INVALID);
  EXPECT(cqlrec_prof_enable(0) == CQLREC_OK);
  EXPECT(cqlrec_prof_select(0xFFFFFFFFu) == CQLREC_OK);
  EXPECT(cqlrec_set_concurrency(1) == CQLREC_OK);
  EXPECT(cqlrec_abi_version() == CQLREC_ABI_VERSION);
  EXPECT(cqlrec_aux_stream(-1) == nullptr && cqlrec_aux_stream(CQLREC_AUX_STREAMS) == nullptr);
  EXPECT(cqlrec_aux_stream(0) == nullptr);       // before cqlrec_runtime_init (which needs a GPU)
  EXPECT(cqlrec_runtime_probe_count() == 0);
}

// every entry point that takes the embedding width refuses d = 96 and d = 0 -- with every other argument acceptable, so it is
// the width that is refused -- in front of any launch (this build has no device code: a launch would fail)
static void unsupported_widths() {
  std::vector<uint16_t> h(64 * 256);
  std::vector<float> f(64 * 256);
  std::vector<int32_t> i32(4096);
  std::vector<int64_t> i64(4096);
  std::vector<unsigned char> wsv(1 << 22);
  void* ws = wsv.data();
  const int64_t wb = (int64_t)wsv.size();
  uint16_t* hp = h.data();
  float* fp = f.data();
  int32_t* ip = i32.data();
  int64_t* lp = i64.data();
  cqlrec_layout lay;
  for (int32_t d : {96, 0}) {
#define REFUSED(call)                                                                  \
  do {                                                                                 \
    cqlrec_layout_make(8, 128, nullptr); /* leaves another text in the error buffer */ \
    EXPECT((call) == CQLREC_ERR_INVALID);                                              \
    EXPECT(strstr(cqlrec_last_error(), "unsupported") != nullptr);                     \
  } while (0)
    REFUSED(cqlrec_layout_make(100, d, &lay));
    REFUSED(cqlrec_gather_pool_fwd(hp, lp, ip, ip, nullptr, 0, 8, 8, d, fp, hp, ip, nullptr));
    REFUSED(cqlrec_gather_pool_bwd(fp, lp, ip, ip, nullptr, 0, 8, 8, d, fp, nullptr));
    REFUSED(cqlrec_gather_pool_bwd_prepare(lp, ip, ip, nullptr, 0, 8, 8, d, 64, ws, wb, nullptr));
    REFUSED(cqlrec_gather_pool_bwd_apply(fp, 8, 8, d, 64, ws, wb, fp, nullptr));
    REFUSED(cqlrec_gather_pool_bwd_sorted(fp, lp, ip, ip, nullptr, 0, 8, 8, d, 64, ws, wb, fp, nullptr));
    REFUSED(cqlrec_linear_bf16(hp, hp, fp, 8, d, 1, fp, hp, nullptr));
    REFUSED(cqlrec_encoder_fwd(hp, hp, fp, hp, fp, 8, d, hp, hp, nullptr));
    REFUSED(cqlrec_encoder_bwd(fp, hp, hp, hp, hp, 8, d, ws, wb, fp, fp, fp, fp, fp, nullptr));
    REFUSED(cqlrec_qhead_fwd(hp, 8, hp, fp, 64, d, CQLREC_QHEAD_LSE, ws, wb, fp, nullptr, fp, nullptr));
    REFUSED(cqlrec_qhead_fwd(hp, 8, hp, fp, 64, d, CQLREC_QHEAD_ARGMAX, ws, wb, fp, ip, nullptr, nullptr));
    REFUSED(cqlrec_gather_dot(hp, hp, fp, ip, 8, d, fp, nullptr));
    REFUSED(cqlrec_qhead_bwd(hp, fp, fp, ip, 8, hp, fp, 64, d, 1.f, ws, wb, fp, fp, fp, nullptr));
    REFUSED(cqlrec_qhead_bwd_items(hp, fp, fp, ip, 8, hp, fp, 64, d, 1.f, ws, wb, fp, fp, nullptr));
    REFUSED(cqlrec_qhead_bwd_states(hp, fp, fp, ip, 8, hp, fp, 64, d, 1.f, ws, wb, fp, nullptr));
    REFUSED(cqlrec_qhead_fwd_lse_dh(hp, 8, hp, fp, 64, d, ws, wb, fp, fp, nullptr));
    REFUSED(cqlrec_qhead_dh_finish(ws, 8, 64, d, fp, fp, ip, hp, 1.f, fp, nullptr));
    REFUSED(cqlrec_score_topk(hp, 8, hp, fp, 64, d, nullptr, nullptr, nullptr, nullptr, 4, ws, wb, ip, fp, ip, nullptr));
    REFUSED(cqlrec_score_topk_phase(hp, 8, hp, fp, 64, d, nullptr, nullptr, nullptr, nullptr, 4, ws, wb, ip, fp, ip,
                                    CQLREC_TOPK_SCORE, nullptr));
    REFUSED(cqlrec_item_norms(hp, 64, d, fp, nullptr));
    REFUSED(cqlrec_item_knn(hp, fp, 64, d, ip, 8, nullptr, 64, CQLREC_SIM_DOT, 4, ws, wb, ip, fp, ip, nullptr));
    REFUSED(cqlrec_pairs_topk(hp, hp, fp, 64, d, lp, ip, nullptr, 8, nullptr, nullptr, 4, ws, wb, fp, ip, fp, ip, nullptr));
#undef REFUSED
    // the width only selects a form here (d = 128 has one of its own): nothing to refuse, nothing launched, "no form"
    int32_t form = 7;
    EXPECT(cqlrec_topk_seen_form(ws, 8, 64, d, 4, &form, nullptr) == CQLREC_OK && form == -1);
    EXPECT(cqlrec_item_knn_ws_bytes(8, 64, d, 4) == 0 && cqlrec_pairs_topk_ws_bytes(8, 64, d, 4) == 0);
  }
}

// the error message buffer is thread-local: concurrent failing calls must not trample each other's text
static void threads() {
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([t] {
      for (int i = 0; i < 200; ++i) {
        cqlrec_layout l;
        if (t & 1) {
          if (cqlrec_layout_make(100, 100 + t, &l) == CQLREC_OK) ++fails;
          if (strstr(cqlrec_last_error(), std::to_string(100 + t).c_str()) == nullptr) ++fails;
        } else if (cqlrec_layout_make(100 + i, 128, &l) != CQLREC_OK) {
          ++fails;
        }
      }
    });
  for (auto& x : th) x.join();
}

// csrc/qde_pieces.h (the cut of the item-side backward) against a direct enumeration of block starts: a block contributes a
// slab piece to group g iff its start lies strictly inside (g T, (g + 1) T) and its range is not empty.  nblk > W is
// included, so empty ranges occur.  Both index widths of the iteration, in block order; any_cut(); the block prologue.
static void qde_pieces_brute_force() {
  for (int32_t G = 1; G <= 12; ++G)
    for (int32_t T = 1; T <= 9; ++T)
      for (int32_t nblk = 1; nblk <= 40; ++nblk) {
        const QdePieces pc = {G, T, nblk};
        const int64_t W = (int64_t)G * T;
        std::vector<int64_t> start(nblk + 1);
        for (int64_t p = 0; p <= nblk; ++p) start[p] = p * W / nblk;
        EXPECT(pc.W() == W && start[0] == 0 && start[nblk] == W);
        bool cut = false, any_piece = false;
        int64_t covered = 0;
        for (int64_t p = 0; p < nblk; ++p) {
          EXPECT(pc.start(p) == start[p] && pc.empty(p) == (start[p + 1] == start[p]));
          const QdePieces::Range rg = pc.range(p);
          EXPECT(rg.u0 == start[p] && rg.nst == start[p + 1] - start[p] && rg.u0 == covered);
          covered += rg.nst;
          if (rg.nst > 0) {
            const QdePieces::Unit u = pc.unit(rg.u0);
            EXPECT(u.t >= 0 && u.t < T && (int64_t)u.g * T + u.t == rg.u0);
          }
          if (p > 0 && start[p] % T != 0) cut = true;
        }
        EXPECT(covered == W);
        for (int32_t g = 0; g < G; ++g) {
          std::vector<int64_t> want, got64, got32;
          for (int64_t p = 0; p < nblk; ++p)
            if (start[p] > (int64_t)g * T && start[p] < ((int64_t)g + 1) * T && start[p + 1] != start[p]) want.push_back(p);
          QDE_FOR_SLAB_PIECES(int64_t, int64_t, pc, (int64_t)g, p) got64.push_back(p);
          QDE_FOR_SLAB_PIECES(uint32_t, uint64_t, pc, (uint32_t)g, p) got32.push_back(p);
          EXPECT(got64 == want && got32 == want);
          any_piece = any_piece || !want.empty();
        }
        EXPECT(pc.any_cut() == cut && cut == any_piece);
      }
  EXPECT(qde_slab_row(3, 256, 17) == 3 * 256 + 17);
  // product, then sum: (1 + 2^-12)^2 rounds to 1 + 2^-11 (a tie, to even), so the sum is 0; an fma would leave 2^-24
  const float a = 1.0f + 0x1p-12f;
  EXPECT(qde_axpy(-(1.0f + 0x1p-11f), a, a) == 0.0f && __builtin_fmaf(a, a, -(1.0f + 0x1p-11f)) == 0x1p-24f);
}

// `host_driver qde_plan B N d n_cu [B N d n_cu ...]`: one line "form G T W grid cut" per shape, for
// tests/test_step_phase_geometry_cpu.py to hold tests/helpers.qde_geometry to
static int print_qde_plans(int argc, char** argv) {
  if ((argc - 2) % 4 != 0) return 2;
  for (int i = 2; i + 3 < argc; i += 4) {
    const int d = atoi(argv[i + 2]);
    const QdePlan pl = qde_plan(atoll(argv[i]), atoll(argv[i + 1]), d, atoi(argv[i + 3]));
    char form[32];
    if (pl.form == QDE_FORM_GENERIC) snprintf(form, sizeof form, "qde_kernel<%d>", d);
    else snprintf(form, sizeof form, "qde%d", pl.form);
    printf("%s %d %d %lld %d %d\n", form, pl.pc.G, pl.pc.T, (long long)pl.pc.W(), pl.pc.nblk, pl.pc.any_cut() ? 1 : 0);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "qde_plan") == 0) return print_qde_plans(argc, argv);
  qde_pieces_brute_force();
  layouts();
  workspace_sizes();
  refused_calls();
  unsupported_widths();
  threads();
  if (fails) {
    fprintf(stderr, "host_driver: %d expectation(s) failed\n", fails);
    return 1;
  }
  printf("host_driver: ok\n");
  return 0;
}
