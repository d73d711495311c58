// K11 — sl_linear_bf16x3: the towers' linear layers as split-bf16 x3 GEMMs on the bf16 matrix cores (gemm_bf16x3.hpp) with
// the epilogue of encoder_epilogue.hpp, and the split itself (sl_split_bf16: fp32 -> hi / lo bf16 planes).
#include "encoder_epilogue.hpp"

using namespace sl;

SL_API size_t sl_split_elems(int64_t R, int64_t K) { return (R < 0 || K < 0) ? 0 : gemm3::split_elems(R, K); }

SL_API int sl_split_bf16(const float* d_x, const float* d_row_scale, int64_t R, int64_t K, uint16_t* d_split, void* stream) {
  SL_REQUIRE(R >= 0 && K >= 0, "sl_split_bf16: negative shape");
  if (R * K == 0) return 0;
  SL_REQUIRE(d_x && d_split && ((uintptr_t)d_split & 127) == 0, "sl_split_bf16: null or unaligned pointer (128-byte lines)");
  return gemm3::launch_split(d_x, d_row_scale, R, K, d_split, (hipStream_t)stream);
}

SL_API int sl_linear_bf16x3(const uint16_t* d_x_split, int64_t M, int64_t K, const uint16_t* d_w_split, int64_t N,
                            const float* d_bias, int act, const float* d_residual, float* d_out, uint16_t* d_out_split,
                            int64_t ldo, int64_t rows_per_group, int64_t group_stride, int64_t row_offset,
                            const float* d_rowadd, void* stream) {
  SL_REQUIRE(M >= 0 && K >= 0 && N >= 0 && ldo >= N, "sl_linear_bf16x3: bad shape");
  SL_REQUIRE(act >= SL_ACT_NONE && act <= SL_ACT_GELU_TANH, "sl_linear_bf16x3: bad activation %d", act);
  if (M * N == 0) return 0;
  const bool split = d_out_split != nullptr;
  SL_REQUIRE(d_x_split && d_w_split && (d_out || split) && !(d_out && split), "sl_linear_bf16x3: null / ambiguous pointers");
  SL_REQUIRE((((uintptr_t)d_x_split | (uintptr_t)d_w_split | (uintptr_t)d_out_split) & 127) == 0,
             "sl_linear_bf16x3: split matrices must be 128-byte aligned");
  const bool remap = rows_per_group > 0;
  SL_REQUIRE(!(remap && (act != SL_ACT_NONE || d_residual || split)), "sl_linear_bf16x3: row scatter is plain fp32 only");
  SL_REQUIRE(!remap || (M < (1ll << 32) && rows_per_group < (1ll << 32)), "sl_linear_bf16x3: row scatter indexes rows with 32 bits");
  SL_REQUIRE(!(split && d_residual), "sl_linear_bf16x3: split output takes no residual");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_GEMM, st, 2.0 * (double)M * (double)N * (double)K);
  auto run = [&](auto a, auto res, auto map, auto sp) {
    LinearEpi<a(), res(), map(), sp()> epi{d_bias, d_residual, d_out, d_out_split, split_kp(N), ldo, rows_per_group, group_stride, row_offset,
                                           d_rowadd, N, rows_per_group > 1 ? (uint32_t)((1ull << 32) / (uint64_t)rows_per_group) : 0xFFFFFFFFu};
    return gemm3::launch_gemm3_nt(prof, d_x_split, M, d_w_split, N, K, epi, st);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (remap) return run(std::integral_constant<int, SL_ACT_NONE>{}, no, yes, no);
  return with_act(act, [&](auto a) { return split ? run(a, no, no, yes) : d_residual ? run(a, yes, no, no) : run(a, no, no, no); });
}
