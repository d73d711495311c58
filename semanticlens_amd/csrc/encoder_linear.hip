// K11 — sl_linear: the towers' linear layers on the fp32-input MFMA GEMM of gemm_f32.hpp, with bias / GELU / residual
// (and, for the patch embedding, the token scatter + positional add) fused into its epilogue (encoder_epilogue.hpp).
#include "encoder_epilogue.hpp"
#include "gemm_f32.hpp"

using namespace sl;

SL_API int sl_linear(const float* d_x, int64_t M, int64_t K, const float* d_w, int64_t N, const float* d_bias, int act,
                     const float* d_residual, float* d_out, int64_t ldo, int64_t rows_per_group, int64_t group_stride,
                     int64_t row_offset, const float* d_rowadd, void* stream) {
  SL_REQUIRE(M >= 0 && K >= 0 && N >= 0 && ldo >= N, "sl_linear: bad shape");
  SL_REQUIRE(act >= SL_ACT_NONE && act <= SL_ACT_GELU_TANH, "sl_linear: bad activation %d", act);
  if (M * N == 0) return 0;
  SL_REQUIRE(d_x && d_w && d_out, "sl_linear: null pointer");
  const bool remap = rows_per_group > 0;
  SL_REQUIRE(!(remap && (act != SL_ACT_NONE || d_residual)), "sl_linear: row scatter supports neither activation nor residual");
  SL_REQUIRE(!remap || (M < (1ll << 32) && rows_per_group < (1ll << 32)), "sl_linear: row scatter indexes rows with 32 bits");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_GEMM, st, 2.0 * (double)M * (double)N * (double)K);
  auto run = [&](auto a, auto res, auto map) {
    LinearEpi<a(), res(), map()> epi{d_bias, d_residual, d_out, nullptr, 0, ldo, rows_per_group, group_stride, row_offset, d_rowadd, N,
                                     rows_per_group > 1 ? (uint32_t)((1ull << 32) / (uint64_t)rows_per_group) : 0xFFFFFFFFu};
    return gemm::launch_gemm_nt(prof, d_x, M, d_w, N, K, epi, st);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (remap) return run(std::integral_constant<int, SL_ACT_NONE>{}, no, yes);
  return with_act(act, [&](auto a) { return d_residual ? run(a, yes, no) : run(a, no, no); });
}
