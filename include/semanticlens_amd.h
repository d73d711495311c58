/*
 * semanticlens_amd.h — C ABI of libsemanticlens_hip.so (gfx950 / MI355X).
 *
 * The reference (jim-berend/semanticlens v0.2.1) is pure Python and has no FFI;
 * its drop-in boundary is the Python plugin API (Lens / ComponentVisualizer /
 * foundation_models).  This header is the native boundary the
 * build places *behind* that API: every entry point replaces the stock-torch
 * arithmetic of one reference call site, cited per function as
 * `semanticlens/<file>:<line>` (paths relative to the reference root).
 *
 * Conventions
 *  - Plain pointers and sizes only.  Pointers named d_* are DEVICE pointers
 *    (HBM, e.g. torch.Tensor.data_ptr()); h_* are host pointers read during
 *    the call.  Nothing is retained after a call returns.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *    work is enqueued asynchronously on it; no entry point synchronises except
 *    sl_prof_read().
 *  - Return value: 0 (or a non-negative code where documented) on success,
 *    negative SL_E_* on failure; sl_last_error() returns a thread-local message.
 *  - No entry point allocates device memory; scratch is passed in by the caller.  The only object that
 *    outlives a call is the RCCL communicator of sl_comm_init_from_unique_id / sl_comm_destroy.
 *  - Process state: what a call computes depends on its arguments alone, and a few process-wide settings choose HOW
 *    (bit-identical variants, arithmetic mode, profiling).  The entry points that read or write them:
 *    sl_set_reduce_policy (the default cache policy of the reduce calls that pass none: sl_reduce_conv, sl_reduce_tokens,
 *    both *_multi, and a negative field of sl_reduce_*_p), sl_set_option / sl_get_option with the environment variable
 *    SL_OPTIONS (read by the GEMM, K2 and K16 dispatchers), sl_set_gemm_mode (the cosine GEMMs) and sl_prof_enable /
 *    sl_prof_reset / sl_prof_read (every profiled launch).  Setting one while another thread is inside a call that
 *    reads it gives that call the old or the new value.
 *  - Strides are in ELEMENTS.
 */
#ifndef SEMANTICLENS_AMD_H
#define SEMANTICLENS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SL_ABI_VERSION 1

/* error codes */
#define SL_E_INVALID (-1)   /* bad argument (message says which) */
#define SL_E_HIP (-2)       /* a HIP runtime call failed */
#define SL_E_UNSUPPORTED (-3)

/* element types of activation tensors */
#define SL_F32 0
#define SL_F16 1
#define SL_BF16 2

/* aggregation over H*W of a (B,C,H,W) activation — component_visualization/aggregators.py:38-87 */
#define SL_CONV_MAX 0  /* aggregate_conv_max  (:64-87)  */
#define SL_CONV_MEAN 1 /* aggregate_conv_mean (:38-61)  */
#define SL_CONV_SUM 2  /* plain sum over H*W: zennit-crp's max_target="sum" used by the relevance visualizer
                          (component_visualization/relevance_based.py:111,140-145) */

/* aggregation over tokens of a (B,T,F) activation — aggregators.py:90-244 */
#define SL_TOK_MEAN 0    /* aggregate_transformer_mean    (:90-114)  */
#define SL_TOK_ABSMEAN 1 /* aggregate_transformer_absmean (:117-141) */
#define SL_TOK_MAX 2     /* aggregate_transformer_max     (:144-168) */
#define SL_TOK_ABSMAX 3  /* aggregate_transformer_absmax  (:171-195) */
#define SL_TOK_TOKEN 4   /* get_aggregate_transformer_special_token(pos) (:198-244) */

/* tie order of the streaming top-k */
#define SL_TIES_TOTAL 0 /* value desc (NaN first, -0 == +0), then sample id asc — batch/shard invariant */
#define SL_TIES_ATEN 1  /* torch.topk's CPU order on cat([state, batch]) — bit-identical to the reference */

#define SL_MAX_SLOTS 16

const char* sl_last_error(void);
int sl_abi_version(void);
/* number of HIP devices visible, or SL_E_HIP */
/* Variant switches — which of several BIT-IDENTICAL kernel variants a dispatcher picks (0 = its own rule).  The parity tests walk the
 * variants with these; production code never needs them.  Names: "g3_tile" (split-bf16 GEMM tile: 128, 256, 8, 160, 64, 1280),
 * "f32_tile" (fp32-MFMA GEMM: 128, 8), "g3_strip_off" (1: no column-strip split), "colreduce_nw" (K2 waves per task: 4, 8, 16),
 * "bn_policy" (K16 cache policy: 1 plain, 2 non-temporal stores, 3 non-temporal loads and stores; 0: 3 from 206 MB, else 1),
 * "g3_shared" (split-bf16 GEMM tile rule: 1 by makespan on an empty chip, 2 by chip time as for a launch that shares the GPU with
 * another stream; 0: by chip time on any stream but the device's default stream).
 * The environment variable SL_OPTIONS="name=value,..." presets them for a process; an explicit call wins.  No reference counterpart. */
int sl_set_option(const char* name, int64_t value);
int64_t sl_get_option(const char* name); /* -1 for an unknown name */
int sl_device_count(void);

/* ---- K1: spatial reduce of a conv activation -------------------------------------------
 * Replaces `tensor.clone().flatten(2).amax(-1)` / `.mean(-1)` (aggregators.py:61, :87) and
 * the bf16 cast `acts.T.to(bfloat16)` (activation_caching.py:133).
 * d_act: (B,C,S) with element strides (sb,sc,ss); S = H*W flattened (NCHW: sc=S, ss=1;
 * channels_last: sc=1, ss=C).
 * d_cand_bf16 (B,C) u16, may be NULL: aggregated value rounded like the reference does
 *   (to the activation dtype, then to bf16 RNE; NaN -> 0x7FC0).
 * d_out_f32 (B,C), may be NULL: aggregated value before the bf16 cast (what the Python
 *   aggregator returns).  At least one output must be non-NULL. */
int sl_reduce_conv(const void* d_act, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                   int64_t ss, int agg, uint16_t* d_cand_bf16, float* d_out_f32, void* stream);

/* Cache policy of the K1 / K2 streams.  A COLD input streams best with the read-once (nt) policy; an input the
 * previous kernel on the stream wrote microseconds ago is partly still in the 256 MiB Infinity Cache and reads faster
 * with the default policy.  Inputs smaller than nt_min_bytes are read with the default policy; of larger ones the last
 * tail_bytes likewise, the rest with nt.  (0, 0) = everything nt, for inputs known to be cold.  Results do not depend on it.
 *
 * sl_reduce_conv_p / sl_reduce_tokens_p (below) take the policy as the call's last two arguments; a negative field takes
 * the process default.  sl_set_reduce_policy sets that process default, for callers that do not pass a policy; negative
 * values restore the built-in one: the environment (SL_NT_MIN_BYTES, SL_REDUCE_TAIL_MB in MiB, read once), else
 * 256 MiB / 240 MiB, i.e. "the input was just produced" — what a forward hook sees. */
int sl_set_reduce_policy(int64_t nt_min_bytes, int64_t tail_bytes);
/* sl_reduce_conv with the cache policy of this call; sl_reduce_conv(...) is sl_reduce_conv_p(..., -1, -1) */
int sl_reduce_conv_p(const void* d_act, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss, int agg,
                     uint16_t* d_cand_bf16, float* d_out_f32, void* stream, int64_t nt_min_bytes, int64_t tail_bytes);

/* Relevance visualizer (relevance_based.py:112, abs_norm=True -> zennit-crp ChannelConcept.reference_sampling):
 * d_x (B,C) fp32 in place, x[b][:] /= (sum_c |x[b][c]| + eps). */
int sl_abs_norm_rows(float* d_x, int64_t B, int64_t C, float eps, void* stream);

/* ---- K2: token reduce of a transformer activation ---------------------------------------
 * Replaces aggregators.py:114,141,168,195,242.  d_act: (B,T,F), strides (sb,st,sf).
 * `pos` is used by SL_TOK_TOKEN only (python-style negative index allowed). */
int sl_reduce_tokens(const void* d_act, int dtype, int64_t B, int64_t T, int64_t F, int64_t sb, int64_t st,
                     int64_t sf, int agg, int64_t pos, uint16_t* d_cand_bf16, float* d_out_f32, void* stream);
/* with the cache policy of this call (see sl_set_reduce_policy); sl_reduce_tokens(...) is sl_reduce_tokens_p(..., -1, -1) */
int sl_reduce_tokens_p(const void* d_act, int dtype, int64_t B, int64_t T, int64_t F, int64_t sb, int64_t st, int64_t sf, int agg,
                       int64_t pos, uint16_t* d_cand_bf16, float* d_out_f32, void* stream, int64_t nt_min_bytes, int64_t tail_bytes);

/* The same reductions over L activations of ONE shape (the hooked outputs of L identical blocks, activation_caching.py:388-418
 * fires once per hooked layer and batch) in one launch where the component axis is contiguous, tensor by tensor otherwise.
 * h_d_acts: host array of L device pointers; d_cand_bf16: (L, B, C) contiguous.  Cache policy: the process default
 * (sl_set_reduce_policy); nothing tunes these per call, so they have no _p form. */
int sl_reduce_conv_multi(const void* const* h_d_acts, int L, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                         int64_t ss, int agg, uint16_t* d_cand_bf16, void* stream);
int sl_reduce_tokens_multi(const void* const* h_d_acts, int L, int dtype, int64_t B, int64_t T, int64_t F, int64_t sb, int64_t st,
                           int64_t sf, int agg, int64_t pos, uint16_t* d_cand_bf16, void* stream);

/* ---- K3: streaming top-k state (ActMax) --------------------------------------------------
 * State = d_vals (C,k) bf16 bit patterns + d_ids (C,k) int64, sorted best-first per row.
 * sl_actmax_init: activation_caching.py:101-110 (values -0.0, ids -1). */
int sl_actmax_init(uint16_t* d_vals, int64_t* d_ids, int64_t C, int64_t k, void* stream);

/* Merge `nslots` candidate batches into the state under SL_TIES_TOTAL
 * (ActMax.update, activation_caching.py:112-141, for several batches at once).
 * Slot s holds h_slot_rows[s] samples as a (rows,C) bf16 matrix at
 * d_cand + s*slot_stride (elements); sample b of slot s has id
 * h_slot_id_base[s] + b (the per-layer counter of activation_caching.py:410-413). */
int sl_actmax_merge(uint16_t* d_vals, int64_t* d_ids, int64_t C, int64_t k, const uint16_t* d_cand,
                    int64_t slot_stride, const int64_t* h_slot_id_base, const int64_t* h_slot_rows, int nslots,
                    void* stream);

/* One ActMax.update (activation_caching.py:112-141): d_cand (B,C) bf16; sample b has id
 * d_sample_ids[b] (device int64 array) or, when d_sample_ids is NULL, id_base + b.
 * ties = SL_TIES_TOTAL or SL_TIES_ATEN.  SL_TIES_ATEN needs d_ws of
 * sl_actmax_aten_ws_bytes(C,k,B) bytes and k + B <= 16384. */
int sl_actmax_update(uint16_t* d_vals, int64_t* d_ids, int64_t C, int64_t k, const uint16_t* d_cand,
                     const int64_t* d_sample_ids, int64_t id_base, int64_t B, int ties, void* d_ws, size_t ws_bytes,
                     void* stream);
size_t sl_actmax_aten_ws_bytes(int64_t C, int64_t k, int64_t B);
/* SL_TIES_ATEN update of L states (their own component counts h_Cs[l], one k) from L candidate matrices (B, C_l) in ONE launch
 * — every hooked layer of a forward pass merged once per batch instead of once per layer (activation_caching.py:388-418 fires per
 * layer).  h_id_bases: the sample id of each layer's first candidate row (the reference's per-layer counter, :410-413).
 * `_supported`: 1 when (k + B) rows fit the one-wavefront-per-row kernel, else update layer by layer. */
int sl_actmax_update_multi(uint16_t* const* h_d_vals, int64_t* const* h_d_ids, const int64_t* h_id_bases, const int64_t* h_Cs,
                           const uint16_t* const* h_d_cands, int L, int64_t k, int64_t B, void* stream);
int sl_actmax_update_multi_supported(int64_t C, int64_t k, int64_t B);
/* HOST-only (no device, no stream): the n-element row h_vals_bf16 in, the k positions torch.topk's CPU kernel would select
 * (activation_caching.py:140: `torch.topk(all_acts, k, dim=1)`; ATen TopKImpl.h -> libstdc++ partial_sort / nth_element + sort,
 * comparator (isnan(a) && !isnan(b)) || a > b) out, best first.  The restatement SL_TIES_ATEN's kernels evaluate; the host side runs
 * it against the installed torch.topk once per process (a torch / libstdc++ pair with another tie order is reported, not followed). */
int sl_aten_topk_order_host(const uint16_t* h_vals_bf16, int64_t n, int64_t k, int32_t* h_positions);

/* ---- K4: merge R other states (e.g. all-gathered per-rank states) into this one ----------
 * No reference counterpart (the reference is single-process); semantics = SL_TIES_TOTAL
 * top-k of the union.  d_other_vals/ids are (R,C,k). */
int sl_actmax_merge_states(uint16_t* d_vals, int64_t* d_ids, int64_t C, int64_t k, const uint16_t* d_other_vals,
                           const int64_t* d_other_ids, int64_t R, void* stream);

/* ---- K4 with its exchange step: RCCL behind this ABI --------------
 * No reference counterpart: the reference is single-process (no torch.distributed / NCCL call anywhere).  One
 * process per GPU; rank r collects the sample range [r*ceil(N/R), ...) with global ids into its own (C,k) states.
 * The communicator is the ONE object of this library that outlives a call: rank 0 obtains an id
 * (sl_comm_unique_id, 128 bytes, host), hands it to the other processes by any means (the Python host uses the
 * torch.distributed store it was launched with), and every rank calls sl_comm_init_from_unique_id on its current HIP
 * device (ncclCommInitRank: collective).  The library links librccl. */
#define SL_COMM_ID_BYTES 128
int sl_comm_unique_id(uint8_t* h_id);
int sl_comm_init_from_unique_id(const uint8_t* h_id, int world, int rank, void** comm);
int sl_comm_destroy(void* comm);
int sl_comm_info(void* comm, int* world, int* rank, int* device);
/* ncclAllGather of nbytes per rank: d_recv (world * nbytes) receives rank r's block at r * nbytes. */
int sl_comm_allgather(void* comm, const void* d_send, void* d_recv, int64_t nbytes, void* stream);
/* in-place ncclAllReduce of n elements (the sharded K5 gather is assembled by a SUM of zero-filled blocks; the
 * bench's max-over-ranks time is a MAX of one double). */
#define SL_COMM_F32 0
#define SL_COMM_F64 1
#define SL_COMM_I64 2
#define SL_COMM_SUM 0
#define SL_COMM_MAX 1
#define SL_COMM_MIN 2
int sl_comm_allreduce(void* comm, void* d_buf, int64_t n, int dtype, int op, void* stream);
/* The cross-rank merge in one call: pack the (C_l,k) states of n_layers layers (h_vals[l] bf16 bits, h_ids[l] int64:
 * host arrays of DEVICE pointers) into d_ws -> ONE ncclAllGather over xGMI -> K4 (SL_TIES_TOTAL top-k of the union) of
 * every layer against the other ranks' blocks, read in place from the gathered buffer.  Afterwards every rank holds the
 * same global states.  d_ws: sl_actmax_allgather_merge_ws_bytes(...) bytes, 16-byte aligned, owned by the caller. */
/* The two local halves on their own (what a caller that brings its own transport uses; the gloo test path does):
 * sl_actmax_pack writes one rank's block — [ids of layer 0..L-1 | values of layer 0..L-1 | zero pad to 16 bytes],
 * sl_actmax_packed_bytes(...) bytes — and sl_actmax_merge_packed folds R such blocks (d_gathered, block r at
 * r * packed_bytes, 8-byte aligned) into the states, leaving block skip_rank (-1: none) out. */
size_t sl_actmax_packed_bytes(int n_layers, const int64_t* h_C, int64_t k);
int sl_actmax_pack(int n_layers, uint16_t* const* h_vals, int64_t* const* h_ids, const int64_t* h_C, int64_t k, void* d_out,
                   void* stream);
int sl_actmax_merge_packed(int n_layers, uint16_t* const* h_vals, int64_t* const* h_ids, const int64_t* h_C, int64_t k,
                           const void* d_gathered, int64_t R, int64_t skip_rank, void* stream);
size_t sl_actmax_allgather_merge_ws_bytes(int n_layers, const int64_t* h_C, int64_t k, int world);
int sl_actmax_allgather_merge(void* comm, int n_layers, uint16_t* const* h_vals, int64_t* const* h_ids, const int64_t* h_C,
                              int64_t k, void* d_ws, size_t ws_bytes, void* stream);

/* ---- K5: concept_db[layer] = embeds[sample_ids] (activation_based.py:387-390) ------------
 * d_emb (N,D) f32, d_ids (n_ids) int64; negative ids wrap (id -1 -> row N-1).  An id
 * outside [-N, N) sets *d_err_flag (int32, may be NULL) to 1 and reads row 0. */
int sl_gather_rows(const float* d_emb, int64_t N, int64_t D, const int64_t* d_ids, int64_t n_ids, float* d_out,
                   int32_t* d_err_flag, void* stream);

/* Sharded form (multi-GPU): d_emb_local holds rows [row_offset, row_offset +
 * n_local) of a table of n_total rows.  Ids index the whole table (negative ids wrap by n_total);
 * rows held elsewhere are written as ZEROS, so a sum (all-reduce) over the shards equals
 * sl_gather_rows on the whole table. */
int sl_gather_rows_shard(const float* d_emb_local, int64_t n_local, int64_t D, const int64_t* d_ids, int64_t n_ids,
                         int64_t row_offset, int64_t n_total, float* d_out, int32_t* d_err_flag, void* stream);

/* ---- K6: similarity_score (scores.py:84-128) ---------------------------------------------
 * Returns the branch taken: 0 row-wise cosine (shapes equal; out (xr,)), 1 normalize(x) @
 * normalize(y) (xc == yr; out (xr,yc)), 2 normalize(x) @ normalize(y)^T (xc == yc; out
 * (xr,yr)); SL_E_INVALID for incompatible shapes (the reference raises ValueError).
 * d_ws: scratch of sl_similarity_ws_bytes(...) bytes.
 * Empty operands follow torch: an output without elements is left alone, and with xc == 0 (every branch contracts over xc)
 * the output is set to zeros; no kernel runs, and d_x / d_y may be NULL in both cases.
 * Arithmetic of the plain branch: split-bf16 x3 on the bf16 matrix cores (|error| ~1e-6 on cosines) when
 * K >= 64, else fp32-input MFMA; SL_GEMM_MODE=f32 in the environment forces the latter. */
int sl_similarity(const float* d_x, int64_t xr, int64_t xc, const float* d_y, int64_t yr, int64_t yc, float* d_out,
                  void* d_ws, size_t ws_bytes, void* stream);
size_t sl_similarity_ws_bytes(int64_t xr, int64_t xc, int64_t yr, int64_t yc);

/* Arithmetic of the cosine GEMMs of sl_similarity(_multi) / sl_redundancy: 1 = split-bf16 x3 (default), 0 = fp32-input
 * MFMA, -1 = as the SL_GEMM_MODE environment variable says.  Process-wide. */
int sl_set_gemm_mode(int mode);

/* One query matrix against L concept matrices — the per-layer loop of `_probe` (lens.py:206-214).  All
 * layers must take similarity_score's plain branch (Q != C_l and K != C_l; otherwise use sl_similarity).
 * h_d_ys / h_d_outs: host arrays of L device pointers ((C_l,K) inputs, (Q,C_l) outputs); h_Cs: host array. */
int sl_similarity_multi(const float* d_x, int64_t Q, int64_t K, const float* const* h_d_ys, const int64_t* h_Cs, int L,
                        float* const* h_d_outs, void* d_ws, size_t ws_bytes, void* stream);
size_t sl_similarity_multi_ws_bytes(int64_t Q, int64_t K, const int64_t* h_Cs, int L);

/* ---- K7: clarity_score (scores.py:18-47): V (C,n,D) -> out (C) ---------------------------- */
int sl_clarity(const float* d_V, int64_t C, int64_t n, int64_t D, float* d_out, void* stream);
/* The per-layer loop of `Lens.eval_clarity` over a concept_db dict (lens.py:391-419) as ONE launch: L layers with the same
 * (n, D) and their own component counts.  h_d_Vs / h_d_outs: host arrays of L device pointers ((C_l,n,D) inputs, (C_l) outputs). */
int sl_clarity_multi(const float* const* h_d_Vs, const int64_t* h_Cs, int L, int64_t n, int64_t D, float* const* h_d_outs,
                     void* stream);

/* ---- K8: redundancy_score (scores.py:50-81): V (Bt,C,D) -> out (Bt) ----------------------- */
int sl_redundancy(const float* d_V, int64_t Bt, int64_t C, int64_t D, float* d_out, void* d_ws, size_t ws_bytes,
                  void* stream);
size_t sl_redundancy_ws_bytes(int64_t Bt, int64_t C, int64_t D);

/* ---- K9: polysemanticity_score (scores.py:131-185): V (C,n,D) -> out (C) float64 ----------
 * Per component: scikit-learn KMeans(n_clusters=2, n_init, random_state) restated on the
 * component's n x n Gram matrix (k-means++ seeding with the caller-supplied random draws,
 * Lloyd iterations with sklearn's tolerance / strict-convergence rules, best-of-n_init by
 * inertia), then 1 - cos(center_1, center_2); rows whose smaller cluster has < 2 samples use
 * the reference's fallback (scores.py:173-184).
 * h_first_center (n_init) int32 and h_rand (n_init,2) float64 are the draws
 * numpy.random.RandomState(random_state) yields for `choice(n, p=uniform)` and
 * `uniform(size=2)` of each init (data independent; produced by the host wrapper).
 * replace_empty_clusters: apply that fallback (the reference's default) or not.
 * d_min_count (C) int32, may be NULL: size of the smaller cluster of the chosen clustering. */
int sl_poly2means(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* h_first_center, int n_init,
                  const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count, void* d_ws,
                  size_t ws_bytes, void* stream);
size_t sl_poly2means_ws_bytes(int64_t C, int64_t n, int64_t D);

/* The same for any `n_clusters` in [2, 16] (scores.py:132,167 forwards the argument to scikit-learn) and n <= 1024:
 * sklearn's k-means++ with 2 + int(ln k) local trials per further centre, Lloyd with relocation of every empty cluster
 * (ascending cluster id, farthest points first), score = 1 - clarity_score of the k centres.  h_rand is
 * (n_init, n_clusters - 1, sl_kmeans_trials(n_clusters)) float64: RandomState.uniform draws in sklearn's order.
 * The same procedure as sl_poly2means (csrc/kmeans.hip writes it once) with its state in the workspace (L2) rather than LDS:
 * for what sl_poly2means does not cover. */
int sl_kmeans_trials(int n_clusters);
int sl_polykmeans(const float* d_V, int64_t C, int64_t n, int64_t D, int n_clusters, const int32_t* h_first_center, int n_init,
                  const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count, void* d_ws,
                  size_t ws_bytes, void* stream);
size_t sl_polykmeans_ws_bytes(int64_t C, int64_t n, int64_t D, int n_clusters, int n_init);

/* ---- K21: facets — the clustering K9's score comes from, and what describe / search need of it -------------------------
 * sl_poly2means_labels / sl_polykmeans_labels: sl_poly2means / sl_polykmeans plus d_labels (C,n) int32: row c is
 * scikit-learn's `labels_` (scores.py:167) of the run component c's score comes from, after the final E-step; cluster j is
 * the j-th seeded centre.  Every other output is bit-identical to the call without labels; same workspace. */
int sl_poly2means_labels(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* h_first_center, int n_init,
                         const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count,
                         int32_t* d_labels, void* d_ws, size_t ws_bytes, void* stream);
int sl_polykmeans_labels(const float* d_V, int64_t C, int64_t n, int64_t D, int n_clusters, const int32_t* h_first_center,
                         int n_init, const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count,
                         int32_t* d_labels, void* d_ws, size_t ws_bytes, void* stream);
/* V (C,n,D) fp32, labels (C,n) int32 -> per component and cluster j in [0,kc):
 *   counts (C,kc) int32, centres (C,kc,D) fp32 = mean of the RAW rows with label j (what scores.py:168 reads as
 *   `cluster_centers_`), clarity (C,kc) fp32 = clarity_score of those rows (may be NULL).
 * A label outside [0,kc) belongs to no facet and is skipped (lets a caller mask samples).
 * count 0: centre row = zeros, clarity NaN.  count 1: clarity NaN.
 * 1 <= kc <= 16, n <= 1024, any D >= 1.  One read of V; results do not depend on the grid; no float atomics. */
int sl_facet_stats(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* d_labels, int n_clusters,
                   float* d_centres, int32_t* d_counts, float* d_clarity, void* stream);

/* ---- K23: silhouette — how many facets a component has (scikit-learn's silhouette_samples / silhouette_score) -----------
 * V (C,n,D) fp32, labels (m,C,n) int32: m label sets over the same samples (the candidate clusterings k = 2..K of
 * polysemanticity_facets(n_clusters="auto")) -> samples (m,C,n) fp64 (may be NULL), mean (m,C) fp64.
 *   cnt_j = #{l: label_l = j};  S_i(j) = sum over l != i with label_l = j of d(i,l)   (l == i is skipped by index)
 *   i in cluster A:  a = S_i(A) / (cnt_A - 1),  b = min over non-empty j != A of S_i(j) / cnt_j,  s_i = (b - a) / max(a, b);
 *   s_i = 0 when cnt_A == 1 or max(a, b) == 0;  mean = mean of s_i over the samples that are in.
 * A label outside [0,n_clusters) takes the sample out, as in sl_facet_stats: it enters no sum, its s_i is NaN, the mean
 * skips it.  Fewer than two non-empty clusters (scikit-learn raises): every s_i and the mean are NaN.
 * metric 0, euclidean: d(i,l) = sqrt(max(H_ii + H_ll - 2 H_il, 0));
 * metric 1, cosine:    d(i,l) = 1 - H_il / (max(sqrt(H_ii), 1e-12) * max(sqrt(H_ll), 1e-12));
 * H = V_c V_c^T accumulated in fp64 from exact fp32 products, (C,n,n) in the workspace: V is read once per call, not once
 * per label set.  1 <= m <= 15, 2 <= n_clusters <= 16, 2 <= n <= 1024, any D >= 1, C <= 65535 per call (C == 0: no-op).
 * All sums are fp64 in a fixed order; results depend on neither the grid nor m; no float atomics. */
size_t sl_silhouette_ws_bytes(int64_t C, int64_t n, int64_t D);
int sl_silhouette(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* d_labels, int m, int n_clusters, int metric,
                  double* d_samples, double* d_mean, void* d_ws, size_t ws_bytes, void* stream);

/* ---- K10: template-difference mean of text embeddings (lens.py:196-199) ------------------
 * E (Q*T,D) read as "(q t) d", E0 (T,D); out (Q,D) = mean_t(E[q,t] - E0[t]). */
int sl_template_mean(const float* d_E, const float* d_E0, int64_t Q, int64_t T, int64_t D, float* d_out,
                     void* stream);

/* ---- K11: primitives of a native CLIP-family transformer tower ----------------
 * The reference's OpenClip.encode_image / encode_text (foundation_models/clip.py:103-135) forward to
 * the third-party open_clip model; these entry points run the same pre-LN transformer arithmetic in
 * fp32 on the device (orchestrated by semanticlens_amd/foundation_models/native_clip.py). */
#define SL_ACT_NONE 0
#define SL_ACT_GELU 1      /* exact erf GELU (torch.nn.GELU()) */
#define SL_ACT_QUICKGELU 2 /* x * sigmoid(1.702 x) (OpenAI CLIP checkpoints) */
#define SL_ACT_GELU_TANH 3 /* tanh approximation (torch gelu(approximate="tanh"); SigLIP towers) */
/* out = act(x W^T + bias) (+ residual): x (M,K), W (N,K) row-major (torch Linear.weight), bias (N) or
 * NULL, residual (M,ldo) or NULL (may alias out), out row stride ldo >= N.  fp32-input MFMA GEMM.
 * Row scatter (patch embedding): when rows_per_group > 0, row r is written to
 *   (r / rows_per_group) * group_stride + row_offset + r % rows_per_group
 * and d_rowadd[(row_offset + r % rows_per_group), :] of a (T,N) table (positional embedding) is added. */
int sl_linear(const float* d_x, int64_t M, int64_t K, const float* d_w, int64_t N, const float* d_bias, int act,
              const float* d_residual, float* d_out, int64_t ldo, int64_t rows_per_group, int64_t group_stride,
              int64_t row_offset, const float* d_rowadd, void* stream);
/* Split matrices: every fp32 value v is carried as hi = bf16(v), lo = bf16(v - hi).  An (R,K) matrix is stored as R
 * rows of 2*Kp bf16 values (Kp = K rounded up to 32, zero padded, the padding must stay zero); each 32-wide k-tile of
 * a row is one 128-byte line [hi(32) | lo(32)]; the buffer is 128-byte aligned and holds sl_split_elems(R,K) uint16.
 * sl_linear_bf16x3 multiplies such operands with three bf16 MFMAs per product (hi*hi + hi*lo + lo*hi, fp32
 * accumulate): fp32-class accuracy at ~2.4x the speed of sl_linear.  Producers (sl_layernorm, sl_attention,
 * sl_patchify, and sl_linear_bf16x3 itself) can emit the split form directly through d_out_split (then d_out is
 * NULL); sl_split_bf16 converts an fp32 matrix (optionally scaling each row first) and writes the zero padding. */
size_t sl_split_elems(int64_t R, int64_t K);
int sl_split_bf16(const float* d_x, const float* d_row_scale, int64_t R, int64_t K, uint16_t* d_split, void* stream);
int sl_linear_bf16x3(const uint16_t* d_x_split, int64_t M, int64_t K, const uint16_t* d_w_split, int64_t N,
                     const float* d_bias, int act, const float* d_residual, float* d_out, uint16_t* d_out_split, int64_t ldo,
                     int64_t rows_per_group, int64_t group_stride, int64_t row_offset, const float* d_rowadd, void* stream);
/* LayerNorm over the last dim (biased variance, like torch.nn.LayerNorm); row strides in elements (fp32 output);
 * d_out_split: (rows, cols) split matrix. */
int sl_layernorm(const float* d_x, int64_t rows, int64_t cols, int64_t x_row_stride, const float* d_gamma,
                 const float* d_beta, float eps, float* d_out, uint16_t* d_out_split, int64_t out_row_stride, void* stream);
/* softmax(q k^T / sqrt(head_dim)) v per (batch, head); d_qkv (B*T, 3*H*head_dim) rows [q | k | v]
 * (torch MultiheadAttention in_proj layout), out (B*T, H*head_dim) fp32 or split; causal != 0 masks keys j > i.
 * head_dim in {32, 64, 72, 80, 88, 96, 104, 128}; any sequence length (K/V stream through LDS in chunks). */
int sl_attention(const float* d_qkv, int64_t B, int64_t T, int64_t H, int64_t head_dim, int causal, float* d_out,
                 uint16_t* d_out_split, void* stream);
/* sl_attention in the split-bf16 x3 arithmetic of sl_linear_bf16x3: both products (q k^T and p v) as a_lo b_hi + a_hi b_lo +
 * a_hi b_hi on the bf16 matrix cores, fp32 softmax and accumulation (~1e-5 relative); same layouts, arguments and head_dims.
 * What NativeClip / NativeSigLip call between two sl_linear_bf16x3 (reference: the attention inside open_clip's towers,
 * foundation_models/clip.py:103-135). */
int sl_attention_bf16x3(const float* d_qkv, int64_t B, int64_t T, int64_t H, int64_t head_dim, int causal, float* d_out,
                        uint16_t* d_out_split, void* stream);
/* Attention pooling with one query per head (the MAP head of SigLIP image towers, clip.py:190-211 SigLipV2 /
 * open_clip attn_pool): out (B, H*head_dim) = softmax(q k_t / sqrt(head_dim)) v over the T tokens of each image.
 * d_q (H*head_dim) is the projected probe; key row (b, t) is d_kv + (b*T + t) * kv_row_stride, its value row v_offset
 * elements further.  head_dim: a multiple of 4 up to 128. */
int sl_attention_pool(const float* d_q, const float* d_kv, int64_t kv_row_stride, int64_t v_offset, int64_t B, int64_t T,
                      int64_t H, int64_t head_dim, float* d_out, void* stream);
/* (B,C,Hi,Wi) image -> (B*(Hi/P)*(Wi/P), C*P*P) patch rows, k = c*P*P + py*P + px (Conv2d weight order). */
int sl_patchify(const float* d_img, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t P, float* d_out,
                uint16_t* d_out_split, void* stream);
/* The same pooling with ONE QUERY PER IMAGE: d_q + b * q_batch_stride is image b's projected query (H*head_dim) — the attention
 * pool of CLIP's ResNet towers (open_clip ModifiedResNet.attnpool behind foundation_models/clip.py:52-62 `OpenClip("RN50", ...)`:
 * the query is the image's mean token).  q_batch_stride 0 = sl_attention_pool. */
int sl_attention_pool_q(const float* d_q, int64_t q_batch_stride, const float* d_kv, int64_t kv_row_stride, int64_t v_offset,
                        int64_t B, int64_t T, int64_t H, int64_t head_dim, float* d_out, void* stream);
/* Token rows of that pool from the NCHW trunk output: d_map (B,C,S) -> d_out (B, S+1, C) with
 * out[b][0] = mean_s map[b][:, s] + pos[0], out[b][1+s] = map[b][:, s] + pos[1+s]; d_pos (S+1, C). */
int sl_tokens_from_map(const float* d_map, int64_t B, int64_t C, int64_t S, const float* d_pos, float* d_out, void* stream);
/* out[g * group_stride_elems + c] = v[c] + add[c] for g < G (class-token row of every image). */
int sl_broadcast_row(const float* d_v, const float* d_add, int64_t G, int64_t group_stride_elems, int64_t N, float* d_out,
                     void* stream);
/* out[b][t][:] = table[ids[b][t]][:] + pos[t][:]  (token + positional embedding of the text tower). */
int sl_embed_tokens(const float* d_table, int64_t vocab, const int64_t* d_ids, int64_t B, int64_t T, int64_t W,
                    const float* d_pos, float* d_out, void* stream);

/* ---- K12: image preprocessing on the device -----------------------------------
 * Replaces the per-sample host transform the reference applies before encode_image
 * (foundation_models/clip.py:157-163 `self.preprocessor(image)`, i.e. open_clip's inference transform:
 * Resize(S, BICUBIC) -> CenterCrop(S) -> ToTensor -> Normalize; "squash": Resize((S,S)) without crop).
 * Bit-identical to Pillow's antialiased resize + torchvision's crop/normalise arithmetic.
 *
 * sl_preprocess_plan is a pure host function: h_hw (B,2) int32 heights/widths of the raw RGB images,
 * h_pixel_offsets (B) byte offset of each image in the packed pixel buffer (NULL: tightly packed in order);
 * writes h_plan (B, SL_PP_PLAN_STRIDE) int64 (upload it unchanged) and h_info[SL_PP_INFO_*].
 * sl_preprocess: d_pixels packed (h,w,3) uint8 images, d_plan the uploaded plan, max_h / coef_bytes from h_info,
 * h_mean/h_std 3 floats each (host); d_out (B,3,S,S) fp32 and/or d_out_u8 (B,S,S,3) resized+cropped bytes
 * (either may be NULL); d_ws of h_info[SL_PP_INFO_WS_BYTES] bytes.  Every refusal (a max_h too tall for the grid
 * included) returns before the first kernel is launched. */
#define SL_PP_SHORTEST 0
#define SL_PP_SQUASH 1
#define SL_PP_BICUBIC 0
#define SL_PP_BILINEAR 1
#define SL_PP_PLAN_STRIDE 16
#define SL_PP_INFO_WS_BYTES 0
#define SL_PP_INFO_COEF_BYTES 1
#define SL_PP_INFO_MAX_H 2
#define SL_PP_INFO_PIXEL_BYTES 3
int sl_preprocess_plan(const int32_t* h_hw, const int64_t* h_pixel_offsets, int64_t B, int S, int resize_mode,
                       int interp, int64_t* h_plan, int64_t* h_info);
int sl_preprocess(const uint8_t* d_pixels, const int64_t* d_plan, int64_t B, int S, int interp, int64_t max_h,
                  int64_t coef_bytes, const float* h_mean, const float* h_std, float* d_out, uint8_t* d_out_u8,
                  void* d_ws, size_t ws_bytes, void* stream);
/* Plan entries for P sub-rectangles of N packed images (host): h_hw (N,2) int32 the full images' heights/widths,
 * h_pixel_offsets (N) their byte offsets (NULL: tightly packed in order), h_index (P) int64 the image of each pair,
 * h_box (P,4) int32 {row1, row2, col1, col2} (ends exclusive; clamped to the image, must stay non-empty).  Each entry reads
 * only its box (plan slot 12: the source row stride in bytes) and sl_preprocess then yields, bit for bit, the transform
 * of the cropped image (`pil.crop((col1, row1, col2, row2))`: crop, then resize).  h_info as for sl_preprocess_plan
 * (SL_PP_INFO_PIXEL_BYTES: the packed buffer's extent). */
int sl_preprocess_plan_rois(const int32_t* h_hw, const int64_t* h_pixel_offsets, int64_t N, const int64_t* h_index,
                            const int32_t* h_box, int64_t P, int S, int resize_mode, int interp, int64_t* h_plan,
                            int64_t* h_info);

/* ---- K13: concept-conditional heatmaps and rendered reference crops ------------
 * sl_render_heatmaps replaces the per-image host loop of the reference's three plot functions
 * (utils/render.py:13-33 _get_square_crop_box, :36-143 vis_lighten_img_border, :146-222 vis_opaque_img_border,
 * :225-267 mystroke, :270-341 crop_and_mask_images): heat = d_rel.sum(1) (crp's attr.heatmap), torchvision
 * gaussian_blur(kernel_size, sigma 0.15 k + 0.35, reflect padding) as two separable fp32 passes, |b| / max|b|
 * (+1e-8 for OPAQUE / LIGHTEN), crp's get_crop_range(crop_th) + the square box, the crop decision, the composite,
 * min-max imgify to uint8 and (OPAQUE / LIGHTEN) the one-pixel stroke and Pillow pastes.  Exact rules: DESIGN.md §K13.
 * d_rel (B,Cin,H,W) and d_img (B,3,H,W) contiguous fp32 (d_img already in display space).  Writes d_heat (B,H,W) the
 * normalised blurred heat (may be NULL), d_box (B,4) int32 {row1, row2, col1, col2} — the square box as computed, ends
 * exclusive and possibly past H / W (slicing clamps) —, d_flags (B) int32 bit 0 = the crop was applied, bit 1 = the
 * rendered mask is non-empty, d_rgb (B,H,W,3) uint8 canvas with the rendered image at its top-left (its extent: the
 * clamped box when bit 0 is set, else H x W).  d_ws: sl_render_ws_bytes(B, H, W) bytes.
 * Refused before any launch: kernel_size even or kernel_size // 2 >= H or W (torch's reflect pad), alpha outside
 * [0, 1], vis_th / crop_th outside [0, 1) (the reference's ValueError texts); kernel_size > 255 or
 * W + kernel_size - 1 > 16384 is SL_E_UNSUPPORTED. */
#define SL_RENDER_CROP 0    /* crop_and_mask_images (:270-341): always cropped, no composite */
#define SL_RENDER_OPAQUE 1  /* vis_opaque_img_border (:146-222) */
#define SL_RENDER_LIGHTEN 2 /* vis_lighten_img_border (:36-143) */
size_t sl_render_ws_bytes(int64_t B, int64_t H, int64_t W);
int sl_render_heatmaps(const float* d_rel, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* d_img, int kernel_size,
                       float vis_th, float crop_th, double alpha, int style, int rf, float* d_heat, int32_t* d_box,
                       int32_t* d_flags, uint8_t* d_rgb, void* d_ws, size_t ws_bytes, void* stream);
/* Start relevance of a conditional backward (zennit-crp CondAttribution with a channel condition, behind the reference's
 * get_max_reference, component_visualization/relevance_based.py:203-246): d_act (B,C,S) strided fp32 (conv (B,C,H,W):
 * S = H*W; tokens (B,T,F): the (B,F,T) view), d_channels (B) int64 device, one channel per row.  rf != 0: d_out = 0
 * except d_out[i, c_i, p_i] = act[i, c_i, p_i] with p_i the FIRST argmax over S (torch.argmax: NaN largest); rf == 0:
 * d_out[i, c_i, :] = act[i, c_i, :], zero elsewhere.  d_out (B,C,S) strided, written in one pass.  A channel outside
 * [0, C) leaves its row zero (callers validate). */
int sl_condition_init(const float* d_act, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss,
                      const int64_t* d_channels, int rf, float* d_out, int64_t ob, int64_t oc, int64_t os, void* stream);

/* ---- K14: crop boxes of heatmaps without a canvas -------------------------------------
 * sl_activation_heat_boxes: P pairs (row d_rows[j], channel d_channels[j]) (int64, device) of a layer output d_act
 * (B,C,S) strided fp32 (sl_condition_init's convention; conv: S = H'*W', prefix 0, grid H' x W'; tokens: the (B,F,T)
 * view, the grid gh x gw starting at token `prefix`).  heat_j = max(bilinear upsample of act[u_j, c_j] to H x W
 * (F.interpolate, align_corners=False; an axis of one cell is copied, not blended with itself), 0); d_box (P,4) int32 = the box sl_render_heatmaps computes for that heat in
 * SL_RENDER_CROP style (blur, |b| / max|b|, crop range, square box; the full image when nothing exceeds crop_th).
 * d_heat (P,H,W) the unblurred heat, written only when non-NULL.  sl_heat_boxes: the same box from a full-resolution
 * d_heat (P,H,W).  d_ws: sl_render_ws_bytes(P, H, W) bytes.  Refused before any launch as sl_render_heatmaps refuses
 * kernel_size and crop_th; out-of-range rows / channels read as an all-zero map (callers validate). */
int sl_activation_heat_boxes(const float* d_act, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss,
                             int64_t prefix, int64_t gh, int64_t gw, const int64_t* d_rows, const int64_t* d_channels,
                             int64_t P, int64_t H, int64_t W, int kernel_size, float crop_th, float* d_heat, int32_t* d_box,
                             void* d_ws, size_t ws_bytes, void* stream);
int sl_heat_boxes(const float* d_heat, int64_t P, int64_t H, int64_t W, int kernel_size, float crop_th, int32_t* d_box,
                  void* d_ws, size_t ws_bytes, void* stream);

/* ---- K16: inference BatchNorm2d with its ReLU / residual add fused in -----------------
 * d_x, d_y (and d_residual): contiguous NCHW fp32 (B,C,HW), 16-byte aligned, distinct buffers; d_mean, d_var, d_scale,
 * d_bias: (C) fp32, read on every launch (nothing is folded or cached).  y = scale * ((x - mean) * rsqrt(var + eps)) + bias,
 * bit for bit what MIOpen's inference BatchNorm writes; relu != 0 applies clamp_min(y, 0) (NaN and the sign of zero as ATen's);
 * the _add_relu form computes clamp_min(y + residual, 0) with y rounded to fp32 first.  C <= 4096, B*C*HW < 2^31. */
int sl_batchnorm_infer(const float* d_x, int64_t B, int64_t C, int64_t HW, const float* d_mean, const float* d_var,
                       const float* d_scale, const float* d_bias, double eps, int relu, float* d_y, void* stream);
int sl_batchnorm_infer_add_relu(const float* d_x, const float* d_residual, int64_t B, int64_t C, int64_t HW,
                                const float* d_mean, const float* d_var, const float* d_scale, const float* d_bias,
                                double eps, float* d_y, void* stream);
/* K19: clamp_min(y_a + y_b, 0), y_a and y_b the BatchNorm values of two tensors of one shape under their own
 * constants and eps, each rounded to fp32 before the add; y_a is the add's left operand.  The tail of a residual block whose
 * shortcut ends in a BatchNorm.  C <= 2048 (two constant tables); anything else as above.  With profiling on, a call leaves two
 * records in SL_PROF_BATCHNORM, the kernel's and an empty one: the slot counts BatchNorm2d evaluations. */
int sl_batchnorm_infer_add_bn_relu(const float* d_xa, const float* d_mean_a, const float* d_var_a, const float* d_scale_a,
                                   const float* d_bias_a, double eps_a, const float* d_xb, const float* d_mean_b,
                                   const float* d_var_b, const float* d_scale_b, const float* d_bias_b, double eps_b, int64_t B,
                                   int64_t C, int64_t HW, float* d_y, void* stream);
/* K18: max_pool2d(clamp_min(y, 0), (kh,kw), (sh,sw), (ph,pw)) of the same y in one pass, bit for bit what ATen's
 * max-pool writes (window clipped to the input, row-major scan, the last NaN of a window wins); no indices, no ceil_mode,
 * dilation 1.  d_x (B,C,H,W), d_y (B,C,OH,OW) with OH = (H + 2 ph - kh) / sh + 1.  k in {2,3}, s in {1,2}, p <= k / 2 per axis,
 * W <= 4096; anything else is SL_E_INVALID. */
int sl_batchnorm_infer_relu_maxpool(const float* d_x, int64_t B, int64_t C, int64_t H, int64_t W, const float* d_mean,
                                    const float* d_var, const float* d_scale, const float* d_bias, double eps, int kh, int kw,
                                    int sh, int sw, int ph, int pw, float* d_y, void* stream);

/* ---- K27: a 64 -> 256 channel 1x1 convolution inside the residual tail ----------------
 * d_x (N,64,HW), d_y and d_identity (N,256,HW): contiguous NCHW fp32, 16-byte aligned, distinct buffers; d_w (256,64) fp32,
 * the Conv2d's weight (no bias).  N*256*HW < 2^31; HW need not be a multiple of anything.  The product is accumulated by
 * v_mfma_f32_16x16x4_f32 in ascending k in `split`'s partial chains, added at the end:
 *   0 one chain; 1 two chains over k [0,32) [32,64); 2 two chains, the 16 steps of four k dealt alternately;
 *   3 four chains over runs of 16 k, added in order; 4 the same, added pairwise; 5 / 6 four chains dealt round-robin, in
 *   order / pairwise.
 * Split 0 reproduced MIOpen's GemmFwd1x1_0_1 bit for bit at (256, 64, 56, 56) (profiles/k27_step0_probe.txt); the others
 * exist for tools/conv_tail_probe.py.  What the GEMM library runs depends on its choice for the shape, so a caller still proves
 * a site on its own input before it trusts it (component_visualization/_bn_fuse.py).
 * sl_conv1x1_64_256 writes the raw product; d_korder, when given, is 64 int32: the input channel that MFMA step s takes in
 * its k slot g is d_korder[4 s + g] (a permutation of 0..63; NULL is ascending).  The other two take split 0 and apply the
 * K16 / K19 tails to the product(s) before anything is stored: clamp_min(bn(W x) + identity, 0) and clamp_min(bn_a(Wa xa) + bn_b(Wb xb), 0), the
 * BatchNorm value rounded to fp32 before the add and bn_a's the left operand.  W and the per-channel tensors are read on
 * every launch. */
int sl_conv1x1_64_256(const float* d_x, const float* d_w, int64_t N, int64_t HW, int split, const int32_t* d_korder, float* d_y,
                      void* stream);
int sl_conv1x1_bn_add_relu(const float* d_x, const float* d_w, const float* d_mean, const float* d_var, const float* d_scale,
                           const float* d_bias, double eps, const float* d_identity, int64_t N, int64_t HW, float* d_y,
                           void* stream);
int sl_conv1x1_bn_add_conv1x1_bn_relu(const float* d_xa, const float* d_wa, const float* d_mean_a, const float* d_var_a,
                                      const float* d_scale_a, const float* d_bias_a, double eps_a, const float* d_xb,
                                      const float* d_wb, const float* d_mean_b, const float* d_var_b, const float* d_scale_b,
                                      const float* d_bias_b, double eps_b, int64_t N, int64_t HW, float* d_y, void* stream);

/* ---- K17: streaming fp32 row top-k — the selection behind label_components / search_components --------
 * No reference counterpart.  State = d_vals (R,k) fp32 + d_ids (R,k) int64, sorted best-first per row; sl_topk_init writes
 * the empty slots (value -inf, id -1).  Order: NaN first, then the larger value, -0.0 == +0.0, equal keys by the smaller id; a
 * real candidate equal to -inf ranks above an empty slot.  The state after a sequence of merges is the top k of everything
 * seen, whatever the cut into tiles and their order.  1 <= k <= 1024; R == 0 is a no-op. */
int sl_topk_init(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, void* stream);
/* Fold a candidate tile into the state: d_cand holds R rows of B >= 1 fp32 columns, row stride ld >= B elements (any 4-byte
 * aligned start); column j has the id id_base + j, ids stay within [0, 2^62].  The tile is fully consumed when the stream
 * reaches the end of this call.  d_ws: sl_topk_merge_ws_bytes(R,k,B) bytes (0 for most shapes: few rows of many columns are
 * split over several wavefronts per row, whose partial selections live there). */
int sl_topk_merge(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_cand, int64_t ld, int64_t B,
                  int64_t id_base, void* d_ws, size_t ws_bytes, void* stream);
size_t sl_topk_merge_ws_bytes(int64_t R, int64_t k, int64_t B);
/* K29: K17's fold of a candidate tile, ranking column j of row r by
 * biased_score(cand[r][j], d_row_bias[r], d_col_bias[j]) = (2 cand - row bias) - column bias in fp32 (csrc/biased_score.hpp; CSLS,
 * the hubness correction behind label_components_csls) instead of by cand[r][j]; the state holds SCORES.  d_row_bias (R,),
 * d_col_bias (B,: the tile's first column is d_col_bias[0]), any 4-byte alignment.  NaN and infinities follow IEEE arithmetic
 * (inf - inf = NaN) and a NaN score ranks first.  Everything else — state layout, sl_topk_init, empty slots, id_base, ld,
 * k <= 1024, split rows and workspace, tiling invariance — is sl_topk_merge's.  A state built by it is merged with
 * sl_topk_merge_states unchanged. */
int sl_topk_merge_biased(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_cand, int64_t ld, int64_t B,
                         int64_t id_base, const float* d_row_bias, const float* d_col_bias, void* d_ws, size_t ws_bytes, void* stream);
/* workspace: sl_topk_merge_ws_bytes(R, k, B) */
/* Fold M explicit entries per row — d_other_vals / d_other_ids (R,M), e.g. another state (M = k) or the states of several
 * layers or ranks side by side — into the state.  Entries with a negative id are empty slots; the caller keeps ids distinct. */
int sl_topk_merge_states(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_other_vals,
                         const int64_t* d_other_ids, int64_t M, void* stream);

/* ---- K20: mutual best matches out of one cosine tile — the selection behind compare_concept_dbs -------
 * No reference counterpart.  Two states of one uint64 per entry: d_row_state (R,) = the best column seen so far for every row,
 * d_col_state (B,) = the best row seen so far for every column.  Entry = (order key of the value << 32) | (0xFFFFFFFF - id);
 * an empty state is all zero bytes (there is no init entry point).  Order: K17's — NaN first, then the larger value,
 * -0.0 == +0.0, equal values by the smaller id.  "Better" is the unsigned maximum of the entries, so the states after a sequence
 * of merges are the maxima of everything seen, bit for bit, whatever the cut into tiles, their order and the scheduling.
 * The entry does not carry a zero's sign or a NaN's payload: they decode as +0.0 and as the canonical quiet NaN.
 * Fold a tile: d_cand holds R rows of B fp32 columns, row stride ld >= B elements (any 4-byte aligned start); row r has the id
 * row_id_base + r, column j the id col_id_base + j, all ids within [0, 2^32 - 2].  The tile is read once and is fully
 * consumed when the stream reaches the end of this call.  R == 0 or B == 0 is a no-op. */
int sl_mutualmax_merge(uint64_t* d_row_state, uint64_t* d_col_state, int64_t R, int64_t B, const float* d_cand, int64_t ld,
                       int64_t row_id_base, int64_t col_id_base, void* stream);
/* Decode n state entries into K17's k = 1 form: d_vals (n,) fp32 and d_ids (n,) int64; an empty entry gives (-inf, -1). */
int sl_mutualmax_finish(const uint64_t* d_state, int64_t n, float* d_vals, int64_t* d_ids, void* stream);

/* K22: per-segment column maxima of a cosine tile (lens.audit_concepts).  State entry (g, j) is d_state[g * state_ld + j], j in [0, B);
   packing, order and decoding are K20's (sl_mutualmax_finish decodes it).  Row r has the id row_id_base + r and belongs to segment
   d_row_seg[r]; a row whose segment is outside [0, G) is ignored.  The rows of a segment need not be adjacent; runs of equal segments are
   what makes it cheap. */
int sl_segmax_merge(uint64_t* d_state, int64_t state_ld, int64_t G, int64_t R, int64_t B, const float* d_cand, int64_t ld,
                    const int32_t* d_row_seg, int64_t row_id_base, void* stream);

/* ---- K24: redundancy groups — which components the redundancy score (reference scores.py:51-81) counts as
 * duplicates of each other.  No reference counterpart.  A group is a connected component of the graph "cosine >= threshold" over the
 * n components of one layer.  State: d_parent (n,) int32, a union-find forest in which a root always hangs under a SMALLER root
 * (parent[x] <= x at every instant; csrc/unionfind.hpp), d_degree (n,) int32, and one int32 status word, raised if a loop ever passed
 * its cap of n + 1 steps; read it once, after the last tile.  n <= 2^31 - 1.
 *
 * sl_unionfind_init writes the empty state: parent[i] = i, degree = 0, status = 0. */
int sl_unionfind_init(int32_t* d_parent, int32_t* d_degree, int32_t* d_status, int64_t n, void* stream);
/* Fold a tile as sl_mutualmax_merge reads one (R rows of B fp32 columns, row stride ld >= B, any 4-byte aligned start): row r has the
 * id row_id_base + r, column c the id col_id_base + c, all within [0, n).  An element is an edge iff row id < column id and
 * v >= threshold (finite): a NaN is never an edge, a tie at the threshold is, the diagonal and what lies left of it are ignored, so a
 * walk over the upper triangle counts every pair once.  Every edge joins the two groups and adds one to both degrees.  A tile with
 * no element right of the diagonal, R == 0 or B == 0 is a no-op without a launch. */
int sl_threshold_union_merge(int32_t* d_parent, int32_t* d_degree, int32_t* d_status, int64_t n, const float* d_cand, int64_t ld,
                             int64_t R, int64_t B, int64_t row_id_base, int64_t col_id_base, float threshold, void* stream);
/* parent[i] = the root above i, idempotent.  Between tiles it keeps the chains short; after the last tile d_parent IS the labels: every
 * component carries the smallest id of its group.  What d_parent holds before that depends on scheduling; the labels and the
 * degrees do not. */
int sl_unionfind_flatten(int32_t* d_parent, int64_t n, int32_t* d_status, void* stream);
/* The optional second pass over the same tiles, with the final labels: d_state (n,) uint32, 0xFFFFFFFF = empty, receives at
 * state[label] the minimum order key (K17's) over the upper-triangle elements whose row and column carry that label. */
int sl_group_min_merge(uint32_t* d_state, const int32_t* d_labels, int64_t n, const float* d_cand, int64_t ld, int64_t R, int64_t B,
                       int64_t row_id_base, int64_t col_id_base, void* stream);
/* d_cohesion[i] = the value of state[labels[i]]: the smallest pairwise cosine inside i's group, NaN for an empty entry (a singleton). */
int sl_group_min_finish(const uint32_t* d_state, const int32_t* d_labels, int64_t n, float* d_cohesion, void* stream);

/* ---- K25: streaming softmax statistics over cosine tiles — the reduction behind label_distribution ------
 * No reference counterpart.  For a row with the candidates c_j and the logits l_j = scale * c_j the state is FOUR doubles,
 * d_state[4 r .. 4 r + 3] = (m, a, b, n): m = max l_j, a = sum exp(l_j - m), b = sum (l_j - m) exp(l_j - m), n = the number of
 * candidates folded (-inf and NaN included).  log_z = m + log a, entropy = log a - b / a (nats), p_j = exp(l_j - log_z).
 * Special values follow torch.logsumexp / torch.softmax in float64 and are told apart by m: a -inf candidate adds to n only; a
 * row that saw a NaN has m = a = b = NaN; one that saw +inf (and no NaN) m = +inf, a = b = NaN; one that saw nothing above -inf
 * m = -inf, a = b = 0.  The rule that merges two states is csrc/softmax_state.hpp's (host-checkable); NaN and +inf are absorbing
 * whatever the order.  No floating-point atomics: the same sequence of calls gives the same bits.  The states after two cuts of
 * the same candidates into tiles agree within the bound of DESIGN.md §K25, not bit for bit.
 *
 * sl_softmax_init writes the empty state (-inf, 0, 0, 0).  d_state is 8-byte aligned; R == 0 is a no-op everywhere. */
int sl_softmax_init(double* d_state, int64_t R, void* stream);
/* Fold a tile read exactly as sl_topk_merge reads one: R rows of B >= 1 fp32 columns, row stride ld >= B elements, any 4-byte
 * aligned start, nothing outside [0, B) of a row touched.  scale must be finite and > 0 (and scale * log2 e a normal fp32 number).
 * d_ws: sl_softmax_merge_ws_bytes(R,B) bytes (0 for most shapes: few rows of many columns are split over several wavefronts per
 * row, whose partial states live there and are folded in a fixed order). */
int sl_softmax_merge(double* d_state, int64_t R, const float* d_cand, int64_t ld, int64_t B, double scale, void* d_ws,
                     size_t ws_bytes, void* stream);
size_t sl_softmax_merge_ws_bytes(int64_t R, int64_t B);
/* d_log_z (R,) and d_entropy (R,) float64: (-inf, NaN) for a row that saw nothing above -inf, (+inf, NaN) after a +inf, (NaN, NaN)
 * after a NaN.  d_vals (R,k): K17's sorted values of the same candidates, or NULL when only the statistics are wanted;
 * d_probs[r,i] = exp(scale * d_vals[r,i] - log_z[r]) as fp32, NaN where log_z[r] is not finite, and 0 for an empty slot (i >= n:
 * the state's count tells an empty slot from a real -inf candidate). */
int sl_softmax_finish(const double* d_state, int64_t R, double scale, const float* d_vals, int64_t k, float* d_probs,
                      double* d_log_z, double* d_entropy, void* stream);

/* ---- K26: ranks of given keys among the candidates of cosine tiles — the count behind label_rank ----------
 * No reference counterpart.  State: d_counts (R,T) int64, zero before the first tile.  A key is a (value, id) pair per row and slot:
 * d_key_vals (R,T) fp32 and d_key_ids (R,T) int64, a negative id = unused slot.  A candidate (value, id) orders before a key iff
 * its id differs from the key's and, in K17's order (NaN first, then the larger value, -0.0 == +0.0, equal values by the smaller
 * id), it stands earlier: csrc/rank_order.hpp, host-checkable.  The candidate with the key's own id is never counted, so after
 * every tile of a row was folded a count is the 0-based position the key holds in the sorted row.  Counts are integers: the state
 * after a sequence of merges is the same whatever the cut into tiles, their order and the scheduling. */
#define SL_RANK_MAX_TARGETS 16
/* d_counts (R,T) int64 += per row r and slot t with d_key_ids[r*T+t] >= 0: the number of columns j in [0,B) for which
 * orders_before(key(d_cand[r*ld+j]), id_base+j, key(d_key_vals[r*T+t]), d_key_ids[r*T+t]).  Slots with a negative key id are
 * not touched.  The tile is read exactly as sl_topk_merge reads one: R rows of B >= 1 fp32 columns, row stride ld >= B elements,
 * any 4-byte aligned start, nothing outside [0, B) of a row touched; id_base within [0, 2^62].  1 <= T <= SL_RANK_MAX_TARGETS;
 * R == 0 is a no-op.  Few rows of many columns are split over sl_rank_merge_splits(R,B) wavefronts per row, whose partial counts
 * are added with 64-bit integer atomics: no workspace. */
int sl_rank_merge(int64_t* d_counts, int64_t R, int64_t T, const float* d_cand, int64_t ld, int64_t B, int64_t id_base,
                  const float* d_key_vals, const int64_t* d_key_ids, void* stream);
int64_t sl_rank_merge_splits(int64_t R, int64_t B); /* waves per row the launch uses; 1 for most shapes */

/* ---- K28: the step of an orthogonal matching pursuit over a vocabulary — behind decompose_components ----------
 * No reference counterpart.  Per component x (a row of d_x (C,D) fp32) the pursuit looks for a few rows of d_w (V,D) fp32 whose
 * normalised forms span x / |x|.  A pass over the vocabulary is sl_cosine_nt + sl_topk_merge of the current residuals with k = t + 1
 * (one of t + 1 candidates is not among the t chosen); sl_omp_step then does, in ONE launch, what torch does per step with a gather
 * of (C,t+1,D) rows, a batched Gram product, cholesky, cholesky_solve, a bmm and a subtraction.  Norms, cosines, the factor, the
 * weights and the residual are float64 from the fp32 inputs; the rules are csrc/omp_state.hpp's, host-checkable.
 *
 * State per component, s = the number of terms asked for, 1 <= s <= SL_OMP_MAX_TERMS:
 *   d_ids (C,s) int64        chosen row of d_w per term, in the order chosen; -1 unused
 *   d_chol (C,s(s+1)/2) f64  Cholesky factor of the chosen unit rows' Gram matrix, lower triangle packed row by row
 *   d_rhs (C,s) f64          their dot products with x / |x|
 *   d_coefs (C,s) f64        the least-squares weights after the last accepted term; 0 unused
 *   d_corr (C,s) fp32        the candidate value a term was chosen with; NaN unused
 *   d_explained (C,s) f64    1 - |residual|^2 after each term; an unused slot repeats the last value (0 without a term)
 *   d_n_terms (C,) int32     terms accepted
 *   d_finished (C,) int32    1 once the component has stopped; later steps leave all of its state alone
 *   d_residual (C,D) fp32    the WORKING residual the next pass reads: x / |x| - sum a_i w_i / |w_i|, zeros once finished
 *   d_last (C,D) fp32        the residual to report: written when a component stops and by step s - 1; complete after step s - 1
 * sl_omp_init writes x / |x| into d_residual and the empty state (d_chol and d_rhs need no clearing).  A component that is a zero
 * row or has a non-finite coordinate is finished at once: d_explained and its d_last row NaN, d_residual zeros.
 *
 * sl_omp_step, step t in [0, s), called for t = 0, 1, .., s - 1 in turn.  Candidates: d_cand_vals / d_cand_ids (C,k_cand), k_cand >= t + 1,
 * best first in K17's order, as sl_topk_merge leaves them.  Per unfinished component: take the first candidate whose id lies in
 * [0, V) and is not among the t chosen (any other id is an empty slot and is never used as an index).  The component stops
 * (d_n_terms = t) when there is none, when its value is NaN or <= min_correlation, or when appending its row gives a Cholesky pivot
 * 1 - z.z below SL_OMP_MIN_PIVOT (the row depends linearly on the chosen ones; a row of zero or non-finite norm stops here too).
 * Otherwise the row is appended, the weights solved, the residual recomputed from x — never updated from the previous one — and
 * d_explained[t] written; the component also stops when |residual|^2 <= SL_OMP_RESIDUAL_DONE.  Both constants are design choices.
 * min_correlation in [0, 1).  Rows are read 16 bytes per lane when D % 4 == 0 and d_x, d_w, d_residual, d_last are 16-byte
 * aligned, else 4 bytes per lane; any 4-byte aligned bases work.  No floating-point atomics: the same inputs give the same bits.
 * C == 0 is a no-op. */
#define SL_OMP_MAX_TERMS 16
#define SL_OMP_MIN_PIVOT 1e-10
#define SL_OMP_RESIDUAL_DONE 1e-8
int sl_omp_init(const float* d_x, int64_t C, int64_t D, int64_t s, int64_t* d_ids, double* d_coefs, float* d_corr,
                double* d_explained, int32_t* d_n_terms, int32_t* d_finished, float* d_residual, float* d_last, void* stream);
int sl_omp_step(const float* d_x, int64_t C, int64_t D, const float* d_w, int64_t V, const float* d_cand_vals,
                const int64_t* d_cand_ids, int64_t k_cand, int64_t t, int64_t s, double min_correlation, int64_t* d_ids,
                double* d_chol, double* d_rhs, double* d_coefs, float* d_corr, double* d_explained, int32_t* d_n_terms,
                int32_t* d_finished, float* d_residual, float* d_last, void* stream);

/* normalize(x) @ normalize(y)^T for ANY shapes — x (M,K), y (N,K), out (M,N) — with K6's kernels and arithmetic mode
 * (sl_set_gemm_mode) and none of similarity_score's shape branches: what the tiled top-k probing calls per tile.
 * d_ws: sl_cosine_nt_ws_bytes(M,N,K) bytes. */
int sl_cosine_nt(const float* d_x, int64_t M, const float* d_y, int64_t N, int64_t K, float* d_out, void* d_ws,
                 size_t ws_bytes, void* stream);
size_t sl_cosine_nt_ws_bytes(int64_t M, int64_t N, int64_t K);

/* ---- measurement --------------------------------------------------------------------------
 * When enabled, every launch of a profiled kernel family is bracketed by HIP events on its
 * own stream.  sl_prof_read synchronises those events and returns the totals. */
#define SL_PROF_REDUCE 0 /* K1/K2 reduce kernels */
#define SL_PROF_MERGE 1  /* K3/K4 merge kernels */
#define SL_PROF_GEMM 2   /* K6 cosine GEMM */
#define SL_PROF_GATHER 3
#define SL_PROF_SCORES 4
#define SL_PROF_BATCHNORM 5 /* K16 fused inference BatchNorm; launches = BatchNorm2d evaluations (K19) */
#define SL_PROF_TOPK 6 /* K17 streaming fp32 top-k; K20 mutual best matches; K22 per-segment maxima; K24 redundancy groups; K26 ranks; K28 pursuit steps */
#define SL_PROF_SOFTMAX 7 /* K25 streaming softmax statistics */
#define SL_PROF_NFAM 8
int sl_prof_enable(int on);
int sl_prof_reset(void);
/* total_ms: sum of event-bracketed durations; launches: count; bytes: algorithmic bytes
 * (or flops for SL_PROF_GEMM) summed over those launches */
int sl_prof_read(int family, double* total_ms, int64_t* launches, double* work);

#ifdef __cplusplus
}
#endif
#endif /* SEMANTICLENS_AMD_H */
