/* vqcpc.h -- C ABI of libvqcpc_hip.so: the MI355X (gfx950) kernels of the VQ-CPC encoder training step.
 *
 * The reference (SonyCSLParis/vqcpc-bach) is pure Python/PyTorch and has NO plugin / FFI interface; its "boundary" for
 * this path is the Python class surface.  Each entry point below therefore names the reference
 * tensor expression it replaces (file:line relative to /root/reference).  A maintainer binds them with ctypes
 * (see INTEGRATION.md); vqcpc_bach_amd/hip.py is exactly that binding.
 *
 * Conventions
 *   - every function returns 0 on success or a negative VQCPC_E* code and never throws; vqcpc_last_error() gives the
 *     thread-local message of the last failure;
 *   - all pointers are DEVICE pointers to caller-owned memory (fp32 / int64 / int32 as declared), 16-byte aligned,
 *     row-major; `ld*` arguments are row strides in ELEMENTS; nothing is allocated inside: kernels that need scratch take
 *     a caller-provided workspace whose size comes from the matching *_workspace() query (a pure host function);
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*; NULL = default stream); no hidden
 *     synchronisation; functions are stateless and re-entrant;
 *   - activations are "block-major": row = block * L + token, i.e. the reference's time-first (L, N, E) tensors
 *     transposed to (N, L, E) and flattened.
 */
#ifndef VQCPC_H
#define VQCPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQCPC_ABI_VERSION 2

#define VQCPC_OK 0
#define VQCPC_EINVAL (-1)    /* bad argument (shape, alignment, null pointer) */
#define VQCPC_ELAUNCH (-2)   /* HIP launch / runtime error */
#define VQCPC_EWORKSPACE (-3) /* workspace too small */

/* ------------------------------------------------------------------------------------------------------------------
 * PROCESS-WIDE STATE.  Every compute entry point is a pure function of its arguments, re-entrant and stream-ordered (work is
 * enqueued on the `stream` argument, nothing is synchronised), EXCEPT for the following settings, which are plain
 * process-wide values read at launch time.  They are configuration, not data: set them before the work they apply to is
 * enqueued and do not change them from a second thread while another one launches.
 *   vqcpc_gemm_set_mode        which GEMM ARITHMETIC vqcpc_gemm_* launch: 0 fp32 MFMA / 1 bf16x6 / 8 bf16 (read by vqcpc_gemm_nt,
 *                              _tn, _tn_grouped, _nt_splitk, _nt_relu_mask, _nt_gatebits and by the *_workspace / *_supported /
 *                              *_groupable queries, whose answers belong to the mode they were asked in).  The library has NO
 *                              kernel-selection switch and reads no tuning variable: every other mode value is refused
 *   vqcpc_gemm_set_gradient_products / vqcpc_gemm_gradient_scope   the bf16-pair gradient arithmetic of round 3 (kept for
 *                              comparison): the scope is a counter, opened and closed by ONE thread around its backward pass.
 *                              The f16x3 gradient GEMMs that training uses (vqcpc_gemm_nt_grad / _tn_grad) are explicit entry
 *                              points whose only state -- the per-call-site scale floats -- is caller-owned device memory
 *   vqcpc_relattn_force_general                         A/B switch of the attention dispatch (tests)
 *   vqcpc_rng_salt_set / vqcpc_rng_salt_advance         a DEVICE-side value (one copy per translation unit) XOR-ed into every
 *                              dropout seed: 0 outside a replayed step graph; a captured step sets it in its first node and
 *                              puts it back to 0 in its last, so work enqueued after a replay on the same stream sees 0
 *   vqcpc_last_error                                    thread-local message of the last failing call of the calling thread
 * Several trainers in one process may therefore interleave their steps at STEP granularity, on one thread or on several
 * (tested: tests/test_graphs_gpu.py::test_two_trainers_interleaved_in_one_process_equal_each_run_apart and
 * ::test_two_trainers_stepping_from_two_threads_equal_each_run_apart): the Python host layer serialises training steps with one
 * process-wide lock (vqcpc_bach_amd/graphs.py STEP_LOCK -- torch.autograd runs every backward node of a device on ONE engine
 * thread, so two concurrent backward passes would interleave there whatever the caller's threads do); callers of the C ABI that
 * step from several threads must agree on the settings above.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_abi_version(void);
const char* vqcpc_last_error(void);
/* returns and clears the HIP runtime's last (non-sticky) error of the calling thread: every launch of this library is checked with
 * hipGetLastError(), which would otherwise attribute an earlier failure of SOMEBODY ELSE's runtime call (a rejected stream capture)
 * to the next kernel launched here */
int vqcpc_clear_runtime_error(void);

/* ------------------------------------------------------------------------------------------------------------------
 * Dropout RNG shared by all kernels: keep(seed, i) = (u24(mix32((uint32)i * 0x9E3779B1 + lo(seed) ^ hi(seed))) >= p * 2^24)
 * with mix32(x): x ^= x >> 16; y = mul24(x, 0x6B43A9); y ^= y >> 15; y = mul24(y, 0x52DCE7) + x; y ^= y >> 14 (mul24 = the low 32 bits of
 * the product of the operands' low 24 bits: the full-rate v_mul_u32_u24; round 5 -- rounds 1-4 used the 'lowbias32' finaliser, two
 * quarter-rate 32-bit multiplies per element).
 * vqcpc_dropout_mask writes that keep-mask (1.0f / 0.0f) for i in [0, n) so that tests can reproduce every
 * in-kernel mask (element index conventions are documented per kernel).
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_dropout_mask(float* mask, int64_t n, float p, uint64_t seed, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Token range check -- the `IndexError: index out of range in self` of nn.Embedding
 * (VQCPCB/data_processor/data_processor.py:26-32 tables, looked up at bach_cpc_data_processor.py:55-63), made asynchronous:
 *   clamped[i] = min(max(tokens[i], 0), limits[i % n_voices] - 1);  *flag |= 1 if any id was outside its table.
 * `limits` is a HOST array of n_voices (<= 16) table sizes (V_c + 1 with the mask token); every kernel of this library
 * that indexes by token id consumes the clamped copy, and the caller raises when it next reads `flag`.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_check_tokens(const int64_t* tokens, int64_t n, int n_voices, const int32_t* limits, int64_t* clamped, int32_t* flag,
                       void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused per-voice embedding + input projection + positional concatenation.
 * Replaces BachCPCDataProcessor.embed (VQCPCB/data_processor/bach_cpc_data_processor.py:42-68) followed by
 * input_linear and the two positional concatenations of RelativeTransformerDownscaler.forward
 * (VQCPCB/downscalers/relative_transformer_downscaler.py:104-115).
 *   table  [n_voices][vmax][dlin] : host-side product  E_v . W_in^T + b_in  (so lookup == embed + linear)
 *   chan   [n_voices][pos], event [tokens_per_block / n_voices][pos]
 *   out    [n_rows][d], d = dlin + 2*pos :  out[r] = [ table[v][tokens[r]] | chan[v] | event[e] ],
 *          p = r % tokens_per_block, v = p % n_voices, e = p / n_voices.
 * bwd accumulates d_table / d_chan / d_event (overwritten, deterministic two-stage reduction).
 * event == NULL (d_event == NULL in bwd): rows are [table | chan] only, width dlin + pos -- the teacher's input
 * `cat(linear_to_input_transformer(embed(x)), channel_embeddings)` (teacher_relative.py:63-75).
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_embed_pos_fwd(const int64_t* tokens, int64_t n_rows, int tokens_per_block, int n_voices, const float* table,
                        int vmax, int dlin, const float* chan, const float* event, int pos, float* out, void* stream);
int64_t vqcpc_embed_pos_bwd_workspace(int64_t n_rows, int tokens_per_block, int n_voices, int vmax, int dlin, int pos);
int vqcpc_embed_pos_bwd(const int64_t* tokens, int64_t n_rows, int tokens_per_block, int n_voices, int vmax, int dlin,
                        int pos, const float* g_out, float* d_table, float* d_chan, float* d_event, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* Block-table lookup of the first layer's QKV projection.  The input of the first encoder layer of a block has only
 * vmax * L distinct rows (token id x position), so `in_proj(x)` (multihead_attention_custom.py:171) is computed once on
 * those rows and looked up per token:  out[r][:] = table[tokens[r] * L + r % L][:],  table [vmax * L][C].
 * segsum is its backward: d_table[t * L + p][:] = sum_{r: tokens[r] = t, r % L = p} g[r][:]  (deterministic). */
int vqcpc_block_table_gather(const float* table, const int64_t* tokens, float* out, int64_t M, int L, int vmax, int C,
                             void* stream);
int64_t vqcpc_block_table_segsum_workspace(int64_t M, int L, int vmax, int C);
int vqcpc_block_table_segsum(const float* g, const int64_t* tokens, float* d_table, int64_t M, int L, int vmax, int C,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* the same with g [M][C] in bf16 (configs[4] bf16 path: the first layer's attention backward writes d q | k | v so,
 * vqcpc_relattn16_bwd_b16 with the token indirection): fp32 accumulation of the upcast values, same order -- bit-identical to
 * vqcpc_block_table_segsum on the same values in fp32; half the bytes in. */
int vqcpc_block_table_segsum_b16(const void* g_bf16, const int64_t* tokens, float* d_table, int64_t M, int L, int vmax, int C,
                                 void* workspace, int64_t workspace_bytes, void* stream);

/* Gradient of a plain row gather out[m] = table[idx[m]] (forward = vqcpc_block_table_gather with L = 1) for a table of
 * any size V: the decoder's `source_embeddings(source)` on merged codes and its shifted target-token lookup
 * (VQCPCB/decoders/decoder.py:212-215,439,474-480).  sorted_idx / perm = idx sorted ascending by a STABLE sort and the
 * permutation that sorts it; d_table [V][C] is overwritten (rows no index refers to become 0); sums run in ascending m. */
int vqcpc_embedding_bwd(const float* g, int64_t ldg, const int64_t* sorted_idx, const int64_t* perm, float* d_table, int64_t M,
                        int64_t V, int C, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Product codes (this package's extension; the reference has only the merged table).  A merged code of a product quantiser
 * of ncb codebooks of K codewords is ncb digits, digit j: c_j = (code / K^j) % K (the order of Encoder.merge_codes),
 * V = K^ncb.  Its embedding is the SUM of one row per codebook, so no tensor of V rows exists.
 * Limits (refused with VQCPC_EINVAL): 1 <= ncb <= 4, 1 <= K <= 4096, V + n_extra < 2^31; C a multiple of 4.
 *
 * vqcpc_product_gather: tables [ncb][K][C], idx [M] int64, 1 <= nj <= ncb leading digits take part.
 *   idx[m] < V:              out[m][:] = (res ? res[m][:] + : ) tables[0][c_0][:] + tables[1][c_1][:] + ... + tables[nj-1][c_{nj-1}][:]
 *                            evaluated left to right, every add one separately rounded fp32 add; without res the chain STARTS at
 *                            the first table row (no `0 +`): nj = 1 without res is a bit-exact row copy.
 *   V <= idx[m] < V + n_extra: out[m][:] = extra[idx[m] - V][:], extra [n_extra][C] (the start-of-sentence rows).
 *   res [M][ldr] (ldr >= C) and extra exclude each other; extra != NULL exactly when n_extra > 0.  out [M][ldo], ldo >= C (ldr
 *   and ldo multiples of 4); columns [C, ldo) are never touched.  A row's bits depend on its own index, its res row and the
 *   tables only.  Indices are NOT checked, as in vqcpc_block_table_gather: the caller guarantees 0 <= idx[m] < V + n_extra.
 *
 * vqcpc_product_gather_bwd: its gradient for the tables and the extra rows (d res = g is the caller's).  The caller forms, for
 *   j < nj and every m, the key  j * K + c_j(idx[m])  where idx[m] < V,  ncb * K + (idx[m] - V)  for j = 0 where idx[m] >= V, and
 *   any value >= ncb * K + n_extra (ignored) for j >= 1 where idx[m] >= V; sorted_keys / perm [S], S = nj * M, are the flattened
 *   [nj][M] key array sorted ascending by a STABLE sort and the permutation that sorts it (perm[s] % M is the row of g).
 *   d_tables [ncb][K][C] and d_extra [n_extra][C] are overwritten:
 *     d_tables[j][k][:] = sum of g[m][:] over {m : idx[m] < V, c_j(idx[m]) = k}   (j < nj; codebooks j >= nj become 0)
 *     d_extra[e][:]     = sum of g[m][:] over {m : idx[m] = V + e}
 *   in ascending m, starting from 0; rows nobody refers to become 0.  Deterministic, no floating-point atomics.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_product_gather(const float* tables, const int64_t* idx, const float* res, int64_t ldr, const float* extra, int n_extra,
                         float* out, int64_t ldo, int64_t M, int ncb, int K, int nj, int C, void* stream);
int vqcpc_product_gather_bwd(const float* g, int64_t ldg, const int64_t* sorted_keys, const int64_t* perm, float* d_tables,
                             float* d_extra, int64_t M, int64_t S, int ncb, int K, int n_extra, int C, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * fp32 MFMA GEMMs (v_mfma_f32_32x32x2_f32).  Replace every F.linear / nn.Linear on the path:
 * multihead_attention_custom.py:171,346 (in_proj / out_proj), transformer_custom.py:285 (linear1/linear2),
 * relative_transformer_downscaler.py:132 (output_linear), mlp_upscaler.py:21-34 and their autograd backward.
 *
 * vqcpc_gemm_nt:  C[M,N] = epilogue( A[M,K] . B[N,K]^T )      (forward: B = weight; dgrad: B = weight^T)
 *   epilogue order:  + bias[N] (nullable) -> ReLU (act==1) -> dropout(p, seed; element index m*N+n, scaled 1/(1-p))
 *                    -> * (gate[m,n] > 0 ? gate_scale : 0) (nullable) -> + add[m,n] (+ add2[m,n]) (nullable) -> store.
 *                    add / add2 may alias C element-wise (each element is read before it is written by the same lane).
 * vqcpc_gemm_tn:  dW[N,K] (+)= A[M,N]^T . B[M,K],  db[N] (+)= column sums of A (db nullable)
 *   split over M into partials in `workspace`, then reduced deterministically; accumulate!=0 adds to dW/db.
 * K % 4 == 0, lda/ldb % 4 == 0 required (16-byte vector loads).
 * ------------------------------------------------------------------------------------------------------------------ */
/* GEMM arithmetic: mode 0 = fp32 operands on v_mfma_f32_32x32x2_f32 (bit-exact fp32 fmaf chains);
 * mode 1 = "bf16x6": each fp32 operand is split exactly into 3 bf16 pieces and a product is evaluated with 6 bf16 MFMAs
 * (v_mfma_f32_32x32x16_bf16) and fp32 accumulation -- fp32-class accuracy at 2.67x the fp32 MFMA rate.
 * mode 8 = plain bf16: operands rounded to bf16 (nearest even), ONE bf16 MFMA per product, fp32 accumulation and epilogue
 * (reduced precision; BASELINE configs[4] names it; 128 x 128 tile kernels).  vqcpc_gemm_get_mode returns 0 / 1 / 2.
 * Process-wide; the initial value comes from the environment variable VQCPC_GEMM_MODE (0, 1, or 8; default 0).
 * vqcpc_gemm_set_mode accepts 0, 1 and 8 and refuses every other value (VQCPC_EINVAL; the mode in force stays). */
int vqcpc_gemm_set_mode(int mode);
int vqcpc_gemm_get_mode(void);
/* Gradient arithmetic of the bf16x6 mode -- OPT-IN, default 6 (= the forward's exact split everywhere).  With 3, the
 * 256 x 256-tile GEMMs launched while a gradient scope is open (the trainers open one around loss.backward(), i.e. the
 * input-gradient NT GEMMs and the weight-gradient TN GEMMs of torch.autograd's backward of F.linear) split each operand into
 * TWO bf16 planes by rounding (h = rn(x), m = rn(x - h): |x - h - m| <= 2^-18 |x|) and evaluate hh + hm + mh: three MFMAs
 * per product, ~2^-17 relative per product, fp32 accumulation.  Forward GEMMs (and hence losses and the code assignment)
 * are never affected.  vqcpc_gemm_gradient_scope(1) opens a scope, (0) closes it (nesting counted); process-wide. */
int vqcpc_gemm_set_gradient_products(int products);
int vqcpc_gemm_get_gradient_products(void);
int vqcpc_gemm_gradient_scope(int open);
/* Gradient GEMMs on THREE fp16 MFMAs per product at fp32-class accuracy (round 5; csrc/gemm_grad.hip) -- the dgrad / wgrad of
 * torch.autograd's backward of F.linear (vqcpc_encoder_trainer.py:311-313 `loss.backward()`, transformer_custom.py:279-289,
 * multihead_attention_custom.py:171,346) for the 256 x 256-tile shapes.  Each operand element x of a tensor with the
 * power-of-two scale s is carried as h = rtz_f16(x s) (saturating) and m = rn_f16(x s - h): |x s - h - m| <= 2^-21 |x s|, a
 * product is hh + hm + mh on v_mfma_f32_32x32x16_f16 with fp32 accumulation, the result is multiplied by 2^-(eA + eB).
 * Explicit entry points, no process-wide switch: the caller chooses them for its backward pass (and, with vqcpc_gemm_nt_f16x3 below,
 * for the forward products of a training step; evaluation / inference callers use vqcpc_gemm_nt).
 * `scale_state`: 4 floats per CALL SITE, caller-owned device memory: [0] / [1] = amax |A| / |B| of the PREVIOUS step (read:
 * the scale maps it into [2^12, 2^13)), [2] / [3] = amax of THIS call's operands (atomic max by the kernel; zero them before).
 * vqcpc_grad_scale_roll(state, nsites) moves [2], [3] -> [0], [1] (sites that ran) and zeroes [2], [3] for `nsites`
 * consecutive sites: once per step; vqcpc_grad_amax primes [0] / [1] of a site on its first use (atomic max of |x| into *slot).
 * vqcpc_gemm_nt_grad: C = epilogue(A . B^T) with epilogue none | + add | + add + add2 | gate-bit mask * gate_scale (the forms
 *   of the input-gradient GEMMs); M, N multiples of 256, K of 32 (persistent over the tiles: the caller cuts ragged rounds).
 *   add == C (same pointer and leading dimension, add2 == NULL): C += A . B^T in place, by fp32 atomic adds at the L2 (one add
 *   per element: the value load-add-store gives, without the epilogue's operand loads).  add2 == C (round 6): C += A . B^T + add
 *   the same way -- the form of the query-path input gradient that lands on the kept rows of d x (a strided C).
 * vqcpc_gemm_tn_grad: dW = A^T . B (+ db = column sums of A, fp32 exact), as vqcpc_gemm_tn (accumulate 0 | 1); N, K multiples
 *   of 256, M of 32. */
int vqcpc_gemm_nt_grad_supported(int64_t M, int N, int K);
int vqcpc_gemm_nt_grad(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                       const float* add, int64_t ldadd, const float* add2, int64_t ldadd2, const void* gate_mask,
                       float gate_scale, float* scale_state, void* stream);
/* vqcpc_gemm_nt_grad_splitk: the same product for FEW output tiles and a long K -- the remainder rows of a launch whose 256-tiles
 * do not fill whole rounds of the persistent kernel (139 264 x 256: two rounds + 32 tiles).  `splits` K slices run as one launch
 * (grid = tiles x splits, partial products into `workspace` planes), one pass sums the planes in ascending order and applies the
 * epilogue: + bias, dropout (row0 = global row of the first row of this call, for the element index (row0 + m) * N + c), + add,
 * + add2 (add may be C: in place).  M, N multiples of 256, K / splits a multiple of 32; deterministic. */
int64_t vqcpc_gemm_nt_grad_splitk_workspace(int64_t M, int N, int splits);
int vqcpc_gemm_nt_grad_splitk(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                              int splits, const float* bias, float drop_p, uint64_t seed, int64_t row0, const float* add,
                              int64_t ldadd, const float* add2, int64_t ldadd2, void* workspace, int64_t workspace_bytes,
                              float* scale_state, void* stream);
/* vqcpc_gemm_nt_grad_tail: the same product for the TAIL rows of a ragged launch on 64 x 128 output tiles, one per workgroup (the last
 * 8 192 rows of 139 264 x 256 occupy all 256 CUs; no partial planes, no third round of 256-tiles).  Same arithmetic, product order
 * and epilogue expression as the 256-tile kernel: without dropout a row carries the bits vqcpc_gemm_nt_grad / _f16x3 give it.
 * Epilogue: + bias, dropout (element index (row0 + m) * N + c), + add (may be C: in place), + add2.  M a multiple of 64, N of 128,
 * K of 32.  Replaces the same lines as vqcpc_gemm_nt_grad (transformer_custom.py:279-289, multihead_attention_custom.py:171,346). */
int vqcpc_gemm_nt_grad_tail_supported(int64_t M, int N, int K);
int vqcpc_gemm_nt_grad_tail(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                            const float* bias, float drop_p, uint64_t seed, int64_t row0, const float* add, int64_t ldadd,
                            const float* add2, int64_t ldadd2, float* scale_state, void* stream);
int vqcpc_gemm_tn_grad_supported(int64_t M, int N, int K);
int64_t vqcpc_gemm_tn_grad_workspace(int64_t M, int N, int K);
int vqcpc_gemm_tn_grad(const float* A, int64_t lda, const float* B, int64_t ldb, float* dW, float* db, int64_t M, int N, int K,
                       int accumulate, void* workspace, int64_t workspace_bytes, float* scale_state, void* stream);
/* The same kernel for the FORWARD products of a training step (opt-in: ops.FWD_ARITH / VQCPC_FWD_ARITH=f16x3; the library default and
 * every evaluation / inference call stay on vqcpc_gemm_nt): C = epilogue(A . B^T + bias) with the forward epilogues of vqcpc_gemm_nt
 * that the 256-tile launches use -- act 0: bias | bias + add | bias + dropout + add (F.linear + dropout + residual,
 * transformer_custom.py:279-289); act 1 with mask_out: bias + relu (+ dropout) and the bit mask of the positive outputs
 * (vqcpc_gemm_nt_relu_mask).  Same dropout element index and mask layout as vqcpc_gemm_nt; shapes and scale_state as
 * vqcpc_gemm_nt_grad. */
int vqcpc_gemm_nt_f16x3(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                        const float* bias, int act, float drop_p, uint64_t seed, const float* add, int64_t ldadd, void* mask_out,
                        float* scale_state, void* stream);
/* Round 6 -- PRE-SPLIT ("P4") operands of the f16x3 products.  A P4 image has the shape, leading dimension and BYTES of the fp32 matrix
 * it mirrors: every aligned group of four consecutive contraction elements (16 bytes) holds {h0 h1 | h2 h3 | m0 m1 | m2 m3}, fp16 pairs
 * (element 0 in the low half) of x * 2^e with h = rtz_f16, m = rn_f16(x 2^e - h), e from the tensor's amax as for scale_state.
 * vqcpc_weight_planes_many: every weight of a trainer's flat parameter buffer ONCE per step (descriptor table of
 *   vqcpc_transpose_many: 4 int64 per matrix = offset, rows, cols, first 32 x 32 tile): amax[i] = max |W_i| of this step, `planes` =
 *   P4 of W_i at the same offset (groups along the columns: B operand of the forward x W^T; needs cols % 4 == 0), `planes_t` = P4 of
 *   W_i^T at the same offset of the transposed-weight arena (groups along the rows: B operand of dy W; needs rows % 4 == 0).
 *   Replaces the split of the same 256 x K weight tile by every workgroup for every output tile (2 176 times per 557 056-row launch).
 * vqcpc_gemm_nt_g3_pl: vqcpc_gemm_nt_grad | vqcpc_gemm_nt_f16x3 with B (and optionally A) given as P4 images + the device scalar
 *   their planes were scaled with (pl_amax_b required, pl_amax_a NULL for an fp32 A): same loads, same LDS image, same products in
 *   the same order -- bit-identical to the fp32-operand entry points whenever those run under the same amax
 *   (tests/test_kernels_gpu.py::test_p4_*).  scale_state still receives the amax of an fp32 A.  A P4 A (pl_amax_a != NULL) goes with
 *   these forms only: none | + add | add == C in place | bias | bias + add | bias + dropout + add.  With add + add2, add2 == C, the
 *   gate mask or relu + mask_out the call is refused (VQCPC_EINVAL, nothing is launched): A must be fp32 there.
 * vqcpc_gemm_nt_g3_small: the 64 x 128-tile kernel of vqcpc_gemm_nt_grad_tail as a general entry point -- tail rows of ragged
 *   launches on P4 operands AND whole products too small for 256-tiles (M % 64 == 0, N % 128 == 0, K % 32 == 0: the 3 072 - 12 288-row
 *   products of the student / decoder steps); operands fp32 or P4 (pl_amax_* NULL: fp32); epilogue in the order of vqcpc_gemm_nt:
 *   + bias, relu (act == 1), dropout, * (gate > 0 ? gate_scale : 0), + add (may be C), + add2. */
int vqcpc_weight_planes_many(const float* base, const int64_t* desc, int n, int64_t total_tiles, float* amax, void* planes,
                             void* planes_t, void* workspace, int64_t workspace_bytes, void* stream);     /* workspace: total_tiles floats */
int vqcpc_gemm_nt_g3_pl(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                        const float* bias, int act, float drop_p, uint64_t seed, const float* add, int64_t ldadd, const float* add2,
                        int64_t ldadd2, const void* gate_mask, float gate_scale, void* mask_out, float* scale_state,
                        const float* pl_amax_a, const float* pl_amax_b, void* stream);
int vqcpc_gemm_nt_g3_small(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                           const float* bias, int act, float drop_p, uint64_t seed, int64_t row0, const float* gate, int64_t ldgate,
                           float gate_scale, const float* add, int64_t ldadd, const float* add2, int64_t ldadd2, float* scale_state,
                           const float* pl_amax_a, const float* pl_amax_b, void* stream);
int vqcpc_grad_amax(const float* x, int64_t ld, int64_t rows, int cols, float* amax_slot, void* stream);
int vqcpc_grad_scale_roll(float* state, int nsites, void* stream);
/* the same, and *saturated_count (uint32, device) += the number of (site, operand) pairs whose amax of this step lay beyond the fp16
 * range under the scale the step used -- elements above 65504 / scale were clamped there: the monitor of a scale that lagged by more
 * than its 16-32 x head-room (the trainers warn at the end of an epoch when it is non-zero) */
int vqcpc_grad_scale_roll_counted(float* state, int nsites, void* saturated_count, void* stream);
/* the same for nsites <= 512 with a LOG (round 6; what the trainers call): `monitor` = int32[3 + log_capacity] on the device:
 * [0] += saturated (site, operand) pairs, [1] = rolls of this table so far (its step index, incremented by every call), [2] = steps
 * with at least one saturated pair, [3 + k] = step index of the k-th such step (the first log_capacity of them).  A step whose scale
 * lagged is thereby MARKED: the trainers' epoch() reports the count and the step indices (`f16x3_scale_saturations`), the next step
 * runs under the followed scale.  Head-room: the scale puts the previous step's amax into [2^11, 2^12), fp16 saturates at 65504 =
 * 2^16: a tensor may grow 16 x (up to 32 x) from one step to the next before its largest elements are clamped. */
int vqcpc_grad_scale_roll_logged(float* state, int nsites, void* monitor, int log_capacity, void* stream);
int vqcpc_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N, int K,
                  const float* bias, int act, float drop_p, uint64_t seed, const float* gate, int64_t ldgate,
                  float gate_scale, const float* add, int64_t ldadd, const float* add2, int64_t ldadd2, void* stream);
int64_t vqcpc_gemm_tn_workspace(int64_t M, int N, int K);
/* Deferred reduction of the weight-gradient partial sums: vqcpc_gemm_tn / vqcpc_gemm_tn_bf16 with accumulate == 2 leave their
 * `splits` partial sums in the workspace (dW partials at float offset s * N * K, db partials at splits * N * K + s * N) and
 * vqcpc_reduce_grouped_vec sums many such products in ONE launch (at the end of a backward pass: 17 launches less per CPC step),
 * with the per-element arithmetic of the immediate reduction.  *_deferred_splits returns the split count, or 0 when the product
 * is too small for the float4 reduction (then reduce immediately). */
int vqcpc_gemm_tn_deferred_splits(int64_t M, int N, int K);
int vqcpc_gemm_tn_bf16_deferred_splits(int64_t M, int N, int K);
int vqcpc_reduce_grouped_vec(int n, const void* const* ws, const int64_t* stride, const int* nsplit, void* const* out,
                             const int64_t* count, int accumulate, void* stream);
int vqcpc_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* dW, float* db, int64_t M, int N, int K,
                  int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
/* Grouped weight gradients: n independent products dW_i (+)= A_i^T B_i, db_i (+)= column sums of A_i in a few launches (32
 * problems per launch pair: products + partial-sum reduction).  For the student / decoder steps, whose ~100 weight gradients
 * per backward pass (3072 rows x 512 ... 2048) cannot fill the chip one at a time; torch.autograd issues them one by one
 * (decoders/decoder.py:431-543, student_encoder_trainer.py:256-296), the trainers of this library defer them to the end of
 * loss.backward().  Arrays are HOST arrays of length n (device pointers inside); db[i] may be NULL; a gradient buffer that
 * occurs twice is accumulated in issue order (full-tile problems first, then the ragged ones, each class in the caller's order).  vqcpc_gemm_tn_groupable: the product is one the grouped kernel serves in the
 * current GEMM mode (bf16x6 / rounded-operand modes, shapes that do not take the 256-tile kernel). */
int vqcpc_gemm_tn_groupable(int64_t M, int N, int K);
int64_t vqcpc_gemm_tn_grouped_workspace(int n, const int64_t* M, const int* N, const int* K);
int vqcpc_gemm_tn_grouped(int n, const void* const* A, const int64_t* lda, const void* const* B, const int64_t* ldb,
                          void* const* dW, void* const* db, const int64_t* M, const int* N, const int* K, int accumulate,
                          void* workspace, int64_t workspace_bytes, void* stream);
/* out[C][R] = in[R][C]^T (weight transposes for the dgrad form of vqcpc_gemm_nt) */
int vqcpc_transpose(const float* in, float* out, int R, int C, void* stream);
/* The transposes of n row-major matrices that live in one buffer, in one launch: matrix i = base_in + desc[4 i] with
 * desc[4 i + 1] rows and desc[4 i + 2] columns, its transpose is written at the same offset of base_out; desc[4 i + 3] = number
 * of 32 x 32 tiles of the matrices before it (ascending), total_tiles = their sum over all n.  `desc` is device memory.
 * (dgrad operands W^T of every nn.Linear of a backward pass: the trainers' flat parameter buffer -> a flat arena.) */
int vqcpc_transpose_many(const float* base_in, float* base_out, const int64_t* desc, int n, int64_t total_tiles, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused self-attention with learned relative bias.
 * Replaces MultiheadAttentionCustom.forward :247-343 and SubsampledRelativeAttention.forward
 * (VQCPCB/transformer/subsampled_relative_attention.py:30-122) through its closed form
 *   bias[h,i,j] = q[h,i].e1[h, L-1-(i-j)] (j <= i) | q[h,i].e2[h, j-i] (j > i).
 *   qkv [n_blocks*L][ldq]: q | k | v at column offsets 0, d, 2d; head h = columns [h*hd, (h+1)*hd); q is UNSCALED
 *   e1, e2 [H*L][hd];  ctx [n_blocks*L][ldo] (heads merged);  probs [n_blocks][H][L][L] = softmax BEFORE dropout
 *   dropout element index = ((block*H + h)*L + i)*L + j.
 * bwd: d_qkv [n_blocks*L][ldg] (all 3d columns written), d_e1/d_e2 overwritten (deterministic partials in workspace).
 * ------------------------------------------------------------------------------------------------------------------ */
/* L = 16 and L = 4 run the one-wavefront-per-block kernels; any other L <= 1024 (teacher_relative.py L = 384,
 * auxiliary_decoder_relative.py L = 24 / 96) runs the strip kernels of relattn_x.hip (Lq = Lk, no mask) with identical semantics.
 * vqcpc_relattn_force_general(1) routes every L through the latter (parity tests between the two). */
int vqcpc_relattn_force_general(int on);
int vqcpc_relattn_fwd(const float* qkv, int64_t ldq, const float* e1, const float* e2, float* ctx, int64_t ldo,
                      float* probs, int64_t n_blocks, int L, int H, int hd, float drop_p, uint64_t seed, void* stream);
int64_t vqcpc_relattn_bwd_workspace(int64_t n_blocks, int L, int H, int hd);
int vqcpc_relattn_bwd(const float* d_ctx, int64_t ldo, const float* qkv, int64_t ldq, const float* probs, const float* e1,
                      const float* e2, float* d_qkv, int64_t ldg, float* d_e1, float* d_e2, int64_t n_blocks, int L, int H,
                      int hd, float drop_p, uint64_t seed, void* workspace, int64_t workspace_bytes, void* stream);

/* First-layer variant: q | k | v are rows of the block table of vqcpc_block_table_gather (table [vmax * L][ldt], row of
 * token r of a block = tokens[r] * L + r); the kernels read them through the token indirection from the L2-resident
 * table instead of a gathered (n_blocks * L, 3d) copy.  d_qkv is still per token (its segment sum is the table gradient:
 * vqcpc_block_table_segsum).  L in {16, 4} only; workspace = vqcpc_relattn_bwd_workspace. */
/* bf16-output forms of the L = 16 attention for the bf16 training path (configs[4]): the attention context (forward) and the
 * gradient of the in_proj output (backward) only feed GEMMs there, which read bf16 from HBM; the kernels round to nearest even
 * on the way out instead of writing fp32 for a cast pass.  ctx_b16 [n_blocks*16][ldo], d_qkv_b16 [n_blocks*16][ldg] bf16
 * (leading dimensions in elements); tokens non-NULL: qkv is the first layer's block table.  Workspace of vqcpc_relattn_bwd. */
int vqcpc_relattn16_b16_supported(int L, int H, int hd);
int vqcpc_relattn16_fwd_b16(const float* qkv, int64_t ldq, const int64_t* tokens, const float* e1, const float* e2, void* ctx_b16,
                            int64_t ldo, float* probs, int64_t n_blocks, int H, int hd, float drop_p, uint64_t seed, void* stream);
int vqcpc_relattn16_bwd_b16(const float* d_ctx, int64_t ldo, const float* qkv, int64_t ldq, const int64_t* tokens,
                            const float* probs, const float* e1, const float* e2, void* d_qkv_b16, int64_t ldg, float* d_e1,
                            float* d_e2, int64_t n_blocks, int H, int hd, float drop_p, uint64_t seed, void* workspace,
                            int64_t workspace_bytes, void* stream);
/* the same for any block length the LDS-tiled kernels serve (L in {16, 4}; L = 16 is forwarded to the matrix-core kernels). */
int vqcpc_relattn_b16_supported(int L, int H, int hd);
int vqcpc_relattn_fwd_b16(const float* qkv, int64_t ldq, const float* e1, const float* e2, void* ctx_b16, int64_t ldo,
                          float* probs, int64_t n_blocks, int L, int H, int hd, float drop_p, uint64_t seed, void* stream);
int vqcpc_relattn_bwd_b16(const float* d_ctx, int64_t ldo, const float* qkv, int64_t ldq, const float* probs, const float* e1,
                          const float* e2, void* d_qkv_b16, int64_t ldg, float* d_e1, float* d_e2, int64_t n_blocks, int L,
                          int H, int hd, float drop_p, uint64_t seed, void* workspace, int64_t workspace_bytes, void* stream);
/* all-bf16 forms (no token indirection): qkv_b16 [n_blocks*16][ldq] is the bf16 output of the in_proj GEMM, d_ctx_b16 the bf16
 * output of the out-proj input-gradient GEMM -- the two kernels' dominant streams at half the bytes. */
int vqcpc_relattn16_fwd_b16io(const void* qkv_b16, int64_t ldq, const float* e1, const float* e2, void* ctx_b16, int64_t ldo,
                              float* probs, int64_t n_blocks, int H, int hd, float drop_p, uint64_t seed, void* stream);
int vqcpc_relattn16_bwd_b16io(const void* d_ctx_b16, int64_t ldo, const void* qkv_b16, int64_t ldq, const float* probs,
                              const float* e1, const float* e2, void* d_qkv_b16, int64_t ldg, float* d_e1, float* d_e2,
                              int64_t n_blocks, int H, int hd, float drop_p, uint64_t seed, void* workspace,
                              int64_t workspace_bytes, void* stream);
int vqcpc_relattn_tab_fwd(const float* table, int64_t ldt, const int64_t* tokens, const float* e1, const float* e2, float* ctx,
                          int64_t ldo, float* probs, int64_t n_blocks, int L, int H, int hd, float drop_p, uint64_t seed,
                          void* stream);
int vqcpc_relattn_tab_bwd(const float* d_ctx, int64_t ldo, const float* table, int64_t ldt, const int64_t* tokens,
                          const float* probs, const float* e1, const float* e2, float* d_qkv, int64_t ldg, float* d_e1,
                          float* d_e2, int64_t n_blocks, int L, int H, int hd, float drop_p, uint64_t seed, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* Rectangular, masked variant for the decoder training step (VQCPCB/decoders/decoder.py:431-543,
 * transformer_custom.py:355-386): Lq = r * Lk queries over Lk keys, q / k / v from separate row-major buffers
 * (self-attention: three column blocks of one in_proj output; cross-attention, multihead_attention_custom.py:173-196:
 * q from the target rows, k | v from the memory rows).  With p = i / r,
 *   bias[h,i,j] = q[h,i].e1[h, Lk-1-(p-j)] (j <= p) | q[h,i].e2[h, j-p] (j > p)
 * (SubsampledRelativeAttention.forward with seq_len_tgt = r * seq_len_src, subsampled_relative_attention.py:30-122) and
 * mask = 0 none | 1 causal (keep j <= p) | 2 anticausal (keep j >= p)  (decoder.py:292-308; masked probabilities are 0).
 *   q [n_seq*Lq][ldq], k [n_seq*Lk][ldk], v [n_seq*Lk][ldv] (head h = columns [h*hd, (h+1)*hd), q UNSCALED),
 *   e1, e2 [H*Lk][hd], ctx [n_seq*Lq][ldo], probs [n_seq][H][Lq][Lk] = softmax BEFORE dropout,
 *   dropout element index = ((seq*H + h)*Lq + i)*Lk + j.   Lk <= 1024, hd in {16, 32, 64, 128}.
 * q, k, v, d_ctx, e1 and e2 are 16-byte aligned and ldq, ldk, ldv, ldo multiples of 4 (rows are loaded as float4).
 * Key tiles a strip of queries cannot see under the mask are skipped (half of the causal self-attention).
 * bwd: same mask as fwd; d_q / d_k / d_v written in full (same layouts, own leading dimensions), d_e1 / d_e2 overwritten. */
int vqcpc_relattn_x_fwd(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                        const float* e1, const float* e2, float* ctx, int64_t ldo, float* probs, int64_t n_seq, int Lq,
                        int Lk, int H, int hd, int mask, float drop_p, uint64_t seed, void* stream);
int64_t vqcpc_relattn_x_bwd_workspace(int64_t n_seq, int Lq, int Lk, int H, int hd);
int vqcpc_relattn_x_bwd(const float* d_ctx, int64_t ldo, const float* q, int64_t ldq, const float* k, int64_t ldk,
                        const float* v, int64_t ldv, const float* probs, const float* e1, const float* e2, float* d_q,
                        int64_t ldgq, float* d_k, int64_t ldgk, float* d_v, int64_t ldgv, float* d_e1, float* d_e2,
                        int64_t n_seq, int Lq, int Lk, int H, int hd, int mask, float drop_p, uint64_t seed, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* Query-subsampled variant for the LAST layer of a stack: `output[::F]` (relative_transformer_downscaler.py:125) keeps
 * only positions 0, F, 2F.. and everything after the attention is per-token, so only those queries are evaluated
 * (keys / values still span the block).  q [n_blocks*L/F][ldq] (projected from x[::F], unscaled), kv [n_blocks*L][ldkv]
 * (k | v at columns 0, d), ctx [n_blocks*L/F][ldo], probs [n_blocks][H][L/F][L].  F = 4.
 * Results equal the full layer followed by the row selection; dropped rows have zero gradient in the reference too. */
int vqcpc_relattn_sub_fwd(const float* q, int64_t ldq, const float* kv, int64_t ldkv, const float* e1, const float* e2,
                          float* ctx, int64_t ldo, float* probs, int64_t n_blocks, int L, int F, int H, int hd,
                          float drop_p, uint64_t seed, void* stream);
int64_t vqcpc_relattn_sub_bwd_workspace(int64_t n_blocks, int L, int F, int H, int hd);
int vqcpc_relattn_sub_bwd(const float* d_ctx, int64_t ldo, const float* q, int64_t ldq, const float* kv, int64_t ldkv,
                          const float* probs, const float* e1, const float* e2, float* d_q, int64_t ldgq, float* d_kv,
                          int64_t ldgkv, float* d_e1, float* d_e2, int64_t n_blocks, int L, int F, int H, int hd,
                          float drop_p, uint64_t seed, void* workspace, int64_t workspace_bytes, void* stream);
/* bf16-output forms of the query-subsampled kernels (the bf16 training path): ctx_b16 / d_kv_b16 hold bf16 elements; d_q (1/8 of
 * the gradient bytes, operand of an fp32 GEMM with two residual inputs) stays fp32. */
int vqcpc_relattn_sub_b16_supported(int L, int F, int H, int hd);
int vqcpc_relattn_sub_fwd_b16(const float* q, int64_t ldq, const float* kv, int64_t ldkv, const float* e1, const float* e2,
                              void* ctx_b16, int64_t ldo, float* probs, int64_t n_blocks, int L, int F, int H, int hd,
                              float drop_p, uint64_t seed, void* stream);
int vqcpc_relattn_sub_bwd_b16(const float* d_ctx, int64_t ldo, const float* q, int64_t ldq, const float* kv, int64_t ldkv,
                              const float* probs, const float* e1, const float* e2, float* d_q, int64_t ldgq, void* d_kv_b16,
                              int64_t ldgkv, float* d_e1, float* d_e2, int64_t n_blocks, int L, int F, int H, int hd,
                              float drop_p, uint64_t seed, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused residual + dropout + LayerNorm:  y = LN(x + dropout(r)) * gamma + beta   (eps inside the sqrt, biased var).
 * Replaces transformer_custom.py:282-283 and :288-289.  x has row stride ldx (the [::4] subsample of
 * relative_transformer_downscaler.py:125 is a stride, not a copy); r, y contiguous [M][d].
 * dropout element index = m*d + c.   mean/rstd [M] are saved for the backward.
 * bwd: d_s [M][d] = gradient w.r.t. (x + dropout(r)) = gradient of the x path; d_r = d_s * mask / (1-p) (may alias d_s
 * when p == 0; pass NULL then); d_gamma / d_beta overwritten.
 * r == NULL: `x` is the residual sum s = x0 + dropout(r) itself (formed by the producing GEMM's epilogue: vqcpc_gemm_nt with
 * bias, drop_p, seed and add = x0 uses the same mask, element index m*N + c with N == d) -- forward: y = LN(s); backward
 * with drop_p > 0 and d_r != NULL: d_r = d_s * mask / (1-p) with the mask regenerated from (seed, index), no r stream.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_add_layernorm_fwd(const float* x, int64_t ldx, const float* r, const float* gamma, const float* beta, float* y,
                            float* mean, float* rstd, int64_t M, int d, float eps, float drop_p, uint64_t seed,
                            void* stream);
int64_t vqcpc_add_layernorm_bwd_workspace(int64_t M, int d);
int vqcpc_add_layernorm_bwd(const float* dy, const float* x, int64_t ldx, const float* r, const float* gamma,
                            const float* mean, const float* rstd, float* d_s, float* d_r, float* d_gamma, float* d_beta,
                            int64_t M, int d, float drop_p, uint64_t seed, void* workspace, int64_t workspace_bytes,
                            void* stream);
/* the same two kernels with an extra bf16 copy of the output that feeds GEMMs in the bf16 path (configs[4]):
 * y_bf16 [M][d] = bf16(y); d_r_bf16 [M][d] = bf16(d_r) (bf16(d_s) when drop_p == 0, where d_r == d_s).  NULL = no copy.
 * forward: y may be NULL when y_bf16 is given (the bf16 copy is the only consumer: 6 instead of 10 bytes per element). */
int vqcpc_add_layernorm_fwd_b16(const float* x, int64_t ldx, const float* r, const float* gamma, const float* beta, float* y,
                                void* y_bf16, float* mean, float* rstd, int64_t M, int d, float eps, float drop_p,
                                uint64_t seed, void* stream);
int vqcpc_add_layernorm_bwd_b16(const float* dy, const float* x, int64_t ldx, const float* r, const float* gamma,
                                const float* mean, const float* rstd, float* d_s, float* d_r, void* d_r_bf16, float* d_gamma,
                                float* d_beta, int64_t M, int d, float drop_p, uint64_t seed, void* workspace,
                                int64_t workspace_bytes, void* stream);
/* the s-form (r == NULL) with the residual sum itself in bf16: x_bf16 [M][ldx] bf16, written by the producing GEMM's epilogue
 * (vqcpc_gemm_nt_bf16 with bias, drop_p, seed, a residual operand and a bf16 output only).  Same arithmetic on the upcast values
 * (bit-identical to the fp32-input kernels given the same values); 2 instead of 4 bytes per element in.  configs[4] bf16 path
 * (transformer_custom.py:279-289: norm1 / norm2 of a layer); x_bf16 8-byte aligned, ldx % 4 == 0. */
int vqcpc_layernorm_fwd_xb16(const void* x_bf16, int64_t ldx, const float* gamma, const float* beta, float* y, void* y_bf16,
                             float* mean, float* rstd, int64_t M, int d, float eps, void* stream);
int vqcpc_layernorm_bwd_xb16(const float* dy, const void* x_bf16, int64_t ldx, const float* gamma, const float* mean,
                             const float* rstd, float* d_s, void* d_s_bf16, float* d_r, void* d_r_bf16, float* d_gamma,
                             float* d_beta, int64_t M, int d, float drop_p, uint64_t seed, void* workspace,
                             int64_t workspace_bytes, void* stream);
/* d_s_bf16 [M][d] = bf16(d_s), NULL = none; d_s may be NULL when d_s_bf16 is given: the gradient of the residual branch then exists in
 * bf16 only -- its one consumer is the bf16 residual operand of the next input-gradient GEMM (vqcpc_gemm_nt_bf16, add_bf16). */
/* ... and with the incoming gradient in bf16 too: dy_bf16 [M][d] bf16 (8-byte aligned), written by the epilogue of the input-gradient
 * GEMM that produced it (vqcpc_gemm_nt_bf16 with a bf16 residual operand and a bf16 output only).  Same arithmetic on the upcast
 * values: bit-identical to vqcpc_layernorm_bwd_xb16 given the same values in fp32; 2 instead of 4 bytes per element in.  configs[4]
 * bf16 path: the gradient of the transformer stack's main stream between sub-layers (transformer_custom.py:279-289 under
 * loss.backward(), vqcpc_encoder_trainer.py:311-313). */
int vqcpc_layernorm_bwd_b16io(const void* dy_bf16, const void* x_bf16, int64_t ldx, const float* gamma, const float* mean,
                              const float* rstd, float* d_s, void* d_s_bf16, float* d_r, void* d_r_bf16, float* d_gamma,
                              float* d_beta, int64_t M, int d, float drop_p, uint64_t seed, void* workspace,
                              int64_t workspace_bytes, void* stream);
/* d_gamma == d_beta == NULL in either backward form: the [vqcpc_add_layernorm_bwd_partials(M, d, r != NULL)][2 d] column partials (d gamma | d beta)
 * stay in `workspace` for a later vqcpc_reduce_grouped.  vqcpc_reduce_grouped: n independent reductions out_i[c] (+)= sum over
 * s < nsplit_i of ws_i[s * stride_i + c], c < count_i, 32 per launch (host arrays of device pointers; a repeated output is
 * accumulated in argument order).  The trainers sum the LayerNorm weight / bias partials of a whole backward pass this way
 * (one launch instead of one reduction + one accumulation per LayerNorm). */
int vqcpc_add_layernorm_bwd_partials(int64_t M, int d, int has_r);   /* has_r: the call passes a separate r (two-input form) */
int vqcpc_reduce_grouped(int n, const void* const* ws, const int64_t* stride, const int* nsplit, void* const* out,
                         const int64_t* count, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Product vector quantiser: nearest code per sub-vector + straight-through output + commitment/codebook loss.
 * Replaces ProductVectorQuantizer.forward distances/argmin/one-hot matmul/_loss/STE
 * (VQCPCB/quantizer/vector_quantizer.py:105-148, :72-83) without the (rows, K, D) intermediate.
 *   z [R][D], codebooks [ncb][K][dsub] (D = ncb*dsub), idx [R][ncb] int64, zq_sg [R][D] = z + (q - z), loss [R].
 * Distance order is canonical: d = 0; for t ascending d = d + (z_t - e_t)^2 with separately rounded sub/mul/add;
 * k ascending, strict '<' (first index wins ties) -- bit-identical to oracle/vqcpc_oracle.py:vq_distances_canonical.
 * assign != 0: idx is computed (argmin); assign == 0: idx is an INPUT (label-corruption path, vector_quantizer.py:119-132).
 * squared != 0: loss = (1 + beta) * sum (q - z)^2 computed as q_latent + beta * e_latent;
 * squared == 0: loss = (1 + beta) * || (q - z) + 1e-5 ||_2.
 * bwd: d_z = g_zq + g_loss * d(loss)/dz ; d_codebooks [ncb][K][dsub] = segment-sum of g_loss * d(loss)/dq
 * (the reference trains codebooks by Adam through this gradient; the EMA codebook update the north_star names is the
 * opt-in second quantiser below: vqcpc_vq_ema_stats / vqcpc_vq_commit_bwd / vqcpc_vq_ema_update).
 * Limits (refused with VQCPC_EINVAL): fwd stages one codebook in the LDS, K * dsub <= 36 864 floats (144 KiB); bwd keeps the
 * K x dsub accumulator next to 256 staged rows, (K + 256) * dsub + 256 floats <= 160 KiB, so dsub <= 158 at most (K = 1).
 * zq_sg == loss == NULL (with assign = 1): index-only mode for inference consumers (decoders/decoder.py:327-336,
 * encoder.py:137-159 only read encoding_indices).
 * Ids are NOT checked: vqcpc_vq_fwd with assign == 0, vqcpc_vq_bwd, vqcpc_embed_pos_fwd / _bwd, vqcpc_block_table_gather /
 * _segsum / _segsum_b16 and vqcpc_embedding_bwd dereference by the indices and tokens they are given, so the caller guarantees
 * that every one is in range (0 <= idx < K, 0 <= token < vmax, 0 <= sorted_idx < V, perm a permutation of [0, M)).
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_vq_fwd(const float* z, const float* codebooks, int64_t R, int ncb, int K, int dsub, float beta, int squared,
                 int assign, int64_t* idx, float* zq_sg, float* loss, void* stream);
int64_t vqcpc_vq_bwd_workspace(int64_t R, int ncb, int K, int dsub);
int vqcpc_vq_bwd(const float* z, const float* codebooks, const int64_t* idx, const float* g_zq, const float* g_loss,
                 int64_t R, int ncb, int K, int dsub, float beta, int squared, float* d_z, float* d_codebooks,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* EMA codebooks (quantizer_type 'ema', EMAProductVectorQuantizer; no counterpart in the reference).  The forward search is
 * vqcpc_vq_fwd with beta = 0 (loss = l exactly; the host scales it by beta).
 * ema_stats: stats [ncb][K][1 + dsub], per code the COUNT of rows assigned to it (column 0) and the SUM of their sub-vectors
 *   (columns 1..dsub), from z [R][D] and idx [R][ncb]: a deterministic segment sum (256-row chunks, one owning lane per LDS
 *   cell, rows in ascending order, chunk partials reduced in chunk order; no float atomics), counts exact.  Refuses
 *   R >= 2^24, dsub + 1 > 256 and K * (1 + dsub) floats that do not fit the LDS next to the staged chunk.  A row whose index
 *   is outside [0, K) is skipped, never dereferenced.
 * commit_bwd: d_z = g_zq + g_loss * beta * dl/dz for l = sum (q - z)^2 (squared) or ||(q - z) + 1e-5||; no codebook gradient
 *   and no segment sum.  In the squared form d_z equals what vqcpc_vq_bwd writes for the same inputs, bit for bit.
 * ema_update, in place, per codebook:  N_k <- g N_k + h n_k ;  m_k <- g m_k + h s_k ;  T = sum_k N_k (pairwise tree over K
 *   padded to a power of two: a function of K alone) ;  Nt_k = (N_k + eps) / (T + K eps) * T ;  e_k <- m_k / Nt_k.
 *   cluster_size [ncb][K], ema_sum and codebooks [ncb][K][dsub]; g = float(decay), h = float(1 - decay) rounded on the host. */
int64_t vqcpc_vq_ema_stats_workspace(int64_t R, int ncb, int K, int dsub);
int vqcpc_vq_ema_stats(const float* z, const int64_t* idx, int64_t R, int ncb, int K, int dsub, float* stats, void* workspace,
                       int64_t workspace_bytes, void* stream);
int vqcpc_vq_commit_bwd(const float* z, const float* codebooks, const int64_t* idx, const float* g_zq, const float* g_loss,
                        int64_t R, int ncb, int K, int dsub, float beta, int squared, float* d_z, void* stream);
int vqcpc_vq_ema_update(const float* stats, float* cluster_size, float* ema_sum, float* codebooks, int ncb, int K, int dsub,
                        float g, float h, float eps, void* stream);

/* Dead-code restarts of the EMA codebooks (opt-in: EMAProductVectorQuantizer(restart_threshold=...)); two launches after
 * ema_update, which stays as it is.
 * restart_candidates: cand [ncb][K][dsub], EVERY element written, independent of N.  With
 *       mix(x): x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31     (mod 2^64)
 *       key = mix(seed + (count + 1) * 0x9E3779B97F4A7C15) ;  r = mix(key + (c * K + k + 1) * 0x9E3779B97F4A7C15)
 *   code (c, k) draws row r_glob = r mod (R * world) of the z [R][ncb * dsub] of `world` ranks laid end to end in rank order:
 *   cand[c][k][:] = z[r_glob % R][c * dsub : (c + 1) * dsub] on the rank r_glob / R, and +0.0f on every other rank (so that
 *   the sum over the ranks is the row).  count = step_dev[0] when step_dev is non-NULL, else `step`.  step_dev is the
 *   counter vqcpc_adam_step_dev reads, and this kernel reads the value that Adam launch reads: the counter AFTER
 *   vqcpc_rng_salt_advance has incremented it for the step, i.e. Adam's t of the step (1 for the first).  The host form
 *   passes that same t.  Refuses R * world >= 2^31, world < 1 and rank outside [0, world).
 * ema_restart, in place: for every code with N[c][k] < thr (strict, fp32): e[c][k] = m[c][k] = cand[c][k], N[c][k] = 1 (the
 *   quantiser's initial-state convention); every other cell keeps its bits.  restarts [ncb] int32 is INCREMENTED by the
 *   number of codes restarted (wave ballot + popcount, one integer atomic per workgroup: schedule-independent); the host
 *   zeroes it.  thr = 0 restarts nothing; a negative thr is refused. */
int vqcpc_vq_restart_candidates(const float* z, int64_t R, int ncb, int K, int dsub, uint64_t seed, uint64_t step,
                                const uint64_t* step_dev, int rank, int world, float* cand, void* stream);
int vqcpc_vq_ema_restart(const float* cand, float* cluster_size, float* ema_sum, float* codebooks, int ncb, int K, int dsub,
                         float thr, int32_t* restarts, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * MlpUpscaler middle: h' = SELU(dropout(h))  (VQCPCB/upscalers/mlp_upscaler.py:21-34); element index = flat index.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_dropout_selu_fwd(const float* h, float* out, int64_t n, float drop_p, uint64_t seed, void* stream);
int vqcpc_dropout_selu_bwd(const float* h, const float* g_out, float* g_h, int64_t n, float drop_p, uint64_t seed,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused bilinear scores + InfoNCE + accuracy.  Replaces FksModule.forward (VQCPCB/vqcpc_helper.py:86-98) on the
 * positive and the N negative sets, the reshuffling of vqcpc_encoder_trainer.py:240-263, nce_loss
 * (vqcpc_helper.py:5-29) and the score matrix (:269).
 *   c [B][cdim], W [zdim][cdim][K], z_pos [B][K][zdim], z_neg [B][N][K][zdim]
 *   f_pos [B][K], f_neg [B][K][N] (saved for bwd), loss_b [B] = -sum_k (pos - logsumexp([neg, pos])),
 *   hits [B][K] = (pos > max_n neg) as 0/1.   loss = mean_b loss_b, accuracy[k] = mean_b hits.
 * bwd (g [B] = dLoss/d loss_b): d_c, d_W (deterministic two-stage), d_z_pos, d_z_neg.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_nce_fwd(const float* c, const float* W, const float* z_pos, const float* z_neg, int B, int K, int N, int zdim,
                  int cdim, float* f_pos, float* f_neg, float* loss_b, float* hits, void* stream);
int64_t vqcpc_nce_bwd_workspace(int B, int K, int N, int zdim, int cdim);
int vqcpc_nce_bwd(const float* c, const float* W, const float* z_pos, const float* z_neg, const float* f_pos,
                  const float* f_neg, const float* g, int B, int K, int N, int zdim, int cdim, float* d_c, float* d_W,
                  float* d_z_pos, float* d_z_neg, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Optimiser on one flat fp32 buffer (all parameters of the trainer are views into it; so are the gradients, which is
 * also the RCCL all-reduce bucket).  Replaces nn.utils.clip_grad_norm_(., 5) + torch.optim.Adam.step
 * (VQCPCB/vqcpc_encoder_trainer.py:92,313-314).
 *   vqcpc_sumsq:   out[0] = sum g^2 (double accumulation, deterministic; workspace from vqcpc_sumsq_workspace)
 *   vqcpc_adam_step: coef = min(1, max_norm / (sqrt(sumsq[0]) + 1e-6)) read ON DEVICE (no host sync); g *= coef;
 *                  m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).
 *   grad_scale multiplies g first (1/world_size for a summed all-reduce).
 * ------------------------------------------------------------------------------------------------------------------ */
int64_t vqcpc_sumsq_workspace(int64_t n);
int vqcpc_sumsq(const float* g, int64_t n, float grad_scale, double* out, void* workspace, int64_t workspace_bytes,
                void* stream);
int vqcpc_adam_step(float* p, float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                    int step, float grad_scale, float max_norm, const double* sumsq, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * GRU cell of the CPC context network (CModule.forward, vqcpc_helper.py:54-76: nn.GRU, gate order r | z | n, h0 = 0,
 * dropout on the outputs of every layer but the last).  gi = x W_ih^T + b_ih and gh = h_prev W_hh^T + b_hh come from
 * vqcpc_gemm_nt; these entry points do the gate arithmetic.  gi, gh [B][3H]; h_prev (NULL = zeros), h_out, y_out [B][H];
 *   r = sigmoid(gi_r + gh_r), u = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), h_out = (1 - u) n + u h_prev,
 *   y_out (nullable) = dropout(h_out), element index = idx_base + b*H + c.
 * bwd: dh = d_y * mask (nullable) + d_h (nullable); writes d_gi, d_gh [B][3H] and d_hprev = dh * u (the recurrent part
 * d_gh . W_hh is a vqcpc_gemm_nt with this tensor as its `add` operand).
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_gru_cell_fwd(const float* gi, const float* gh, const float* h_prev, float* h_out, float* y_out, int64_t B, int H,
                       float drop_p, uint64_t seed, uint64_t idx_base, void* stream);
int vqcpc_gru_cell_bwd(const float* gi, const float* gh, const float* h_prev, const float* d_y, const float* d_h, float* d_gi,
                       float* d_gh, float* d_hprev, int64_t B, int H, float drop_p, uint64_t seed, uint64_t idx_base,
                       void* stream);
/* One launch per time step (recurrent product + gate arithmetic fused; H % 64 == 0 -- vqcpc_gru_step_supported):
 * fwd: gh[B][3H] = h_prev W_hh^T + b_hh (h_prev NULL = zeros: gh = b_hh), then the cell of vqcpc_gru_cell_fwd on gi, gh;
 * bwd (step t -> t-1): dh = dgh_next[B][3H] . whh_t[H][3H]^T + dhp[B][H] (+ d_y * mask), then the cell backward of step t-1
 *      (gi, gh, h_prev of THAT step): d_gi, d_gh [B][3H]; dhp is overwritten with dh * u (the next launch's direct term).
 * Replaces one vqcpc_gemm_nt + one gate launch (+ a split-K reduction) per step of nn.GRU (vqcpc_helper.py:54-76). */
int vqcpc_gru_step_supported(int64_t B, int H);
int vqcpc_gru_step_fwd(const float* gi, const float* w_hh, const float* b_hh, const float* h_prev, float* gh, float* h_out,
                       float* y_out, int64_t B, int H, float drop_p, uint64_t seed, uint64_t idx_base, void* stream);
int vqcpc_gru_step_bwd(const float* dgh_next, const float* whh_t, float* dhp, const float* gi, const float* gh,
                       const float* h_prev, const float* d_y, float* d_gi, float* d_gh, int64_t B, int H, float drop_p,
                       uint64_t seed, uint64_t idx_base, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * First layer of the GRU block downscaler (LstmDownscaler.compute_z, lstm_downscaler.py:73-94: g_enc_fwd on the blocks,
 * g_enc_bwd on x.flip(dims=[1]); x = BachCPCDataProcessor.embed, bach_cpc_data_processor.py:24-28: a per-voice table
 * lookup without a positional term).  gi = x W_ih^T + b_ih of nn.GRU's first layer then takes n_voices * vmax distinct
 * rows, so it is computed once on the stacked embedding tables, gi_table [n_voices * vmax][3H], and the step kernels read
 *   gi of row b  =  gi_table[(p % n_voices) * vmax + tokens[b * L + p]][0 .. 3H)
 * for the step at block position p (p = t for the forward stack, L - 1 - t for the flipped one); tokens [B][L] int64,
 * clamped into [0, vmax).  Everything else -- arguments, arithmetic, dropout indices -- is that of the four entry points
 * above: their results are bit-identical when gi holds the gathered rows.  d_gi stays a [B][3H] buffer of the step.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_gru_tok_cell_fwd(const float* gi_table, const int64_t* tokens, int L, int p, int n_voices, int vmax, const float* gh,
                           const float* h_prev, float* h_out, float* y_out, int64_t B, int H, float drop_p, uint64_t seed,
                           uint64_t idx_base, void* stream);
int vqcpc_gru_tok_cell_bwd(const float* gi_table, const int64_t* tokens, int L, int p, int n_voices, int vmax, const float* gh,
                           const float* h_prev, const float* d_y, const float* d_h, float* d_gi, float* d_gh, float* d_hprev,
                           int64_t B, int H, float drop_p, uint64_t seed, uint64_t idx_base, void* stream);
int vqcpc_gru_tok_step_fwd(const float* gi_table, const int64_t* tokens, int L, int p, int n_voices, int vmax, const float* w_hh,
                           const float* b_hh, const float* h_prev, float* gh, float* h_out, float* y_out, int64_t B, int H,
                           float drop_p, uint64_t seed, uint64_t idx_base, void* stream);
int vqcpc_gru_tok_step_bwd(const float* dgh_next, const float* whh_t, float* dhp, const float* gi_table, const int64_t* tokens,
                           int L, int p, int n_voices, int vmax, const float* gh, const float* h_prev, const float* d_y,
                           float* d_gi, float* d_gh, int64_t B, int H, float drop_p, uint64_t seed, uint64_t idx_base,
                           void* stream);
/* Gradient of gi_table from ONE step's d_gi [R][C] (C = 3H): for every v in [0, vmax)
 *   d_table[(p % n_voices) * vmax + v][:]  (accumulate ? += : =)  sum of d_gi[b][:] over the rows b with tokens[b * L + p] == v,
 * rows added in ascending order within 64 row chunks at the most, the chunks in ascending order (no float atomics: two calls
 * give the same bits); a v that no row holds gets 0 (accumulate = 0) or stays (accumulate = 1).  The backward pass calls it
 * once per step: the first visit of a voice writes, later ones accumulate (the embedding backward that nn.GRU's first
 * layer ends in, lstm_downscaler.py:79,84). */
int64_t vqcpc_gru_tok_segsum_workspace(int64_t R, int vmax, int C);
int vqcpc_gru_tok_segsum(const float* d_gi, const int64_t* tokens, int L, int p, int n_voices, int vmax, float* d_table, int64_t R,
                         int C, int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Student (distilled VQ-VAE) step, SURVEY.md section 8 row A23.
 *
 * vqcpc_softmax_ce: one row = one (batch row, masked event, channel) logit vector.
 *   target != NULL        : loss[r] = -log_softmax(logits[r])[target[r]]      utils.categorical_crossentropy (utils.py:24-49)
 *   target_logits != NULL : loss[r] = -sum_v softmax(target_logits[r])[v] log_softmax(logits[r])[v]
 *                                                                  utils.distilled_categorical_crossentropy (utils.py:131-159)
 *   grad [R][V] = d loss[r] / d logits[r] = softmax(logits[r]) - target distribution  (backward = vqcpc_scale_rows).
 * vqcpc_upscale_*: AuxiliaryDecoderRelative.upscale (auxiliary_decoder_relative.py:116-130):
 *   out[(r*f + u)][:] = x[r][:] + emb[u][:]; bwd: dx[r] = sum_u g[r*f+u], d_emb[u] = sum_r g[r*f+u] (f <= 8).
 * ------------------------------------------------------------------------------------------------------------------ */
/* 'same_sequence' negative construction on the device (BachCPCDataloaderGenerator._build_negatives_sameSeq,
 * dataloaders/bach_cpc_dataloader.py:163-181): first (B, blocks_first * tokens_per_block), second likewise, int64 tokens in
 * (tick, voice) order; out (B, blocks_first + blocks_second - 1, blocks_second, tokens_per_block):
 *   out[b][n][k] = first block n (n < blocks_first) | second block j' with j = n - blocks_first, j' = j < k ? j : j + 1.
 * negative_samples = f(x_left, x_right), negative_samples_back = f(x_right, x_left) (:131-132). */
int vqcpc_same_sequence_negatives(const int64_t* first, const int64_t* second, int64_t* out, int64_t B, int blocks_first,
                                  int blocks_second, int tokens_per_block, void* stream);
int vqcpc_softmax_ce(const float* logits, int64_t ld, const int64_t* target, const float* target_logits, int64_t ldt,
                     float* loss, float* grad, int64_t R, int V, void* stream);
int vqcpc_scale_rows(const float* in, const float* g, float* out, int64_t R, int V, void* stream);
int vqcpc_upscale_fwd(const float* x, const float* emb, float* out, int64_t rows, int f, int d, void* stream);
int64_t vqcpc_upscale_bwd_workspace(int64_t rows, int f, int d);
int vqcpc_upscale_bwd(const float* g, float* dx, float* d_emb, int64_t rows, int f, int d, void* workspace,
                      int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * bf16 GEMM path for BASELINE configs[4] (reduced precision; never used for the fp32 headline configuration).
 * Operands are bf16 (uint16 bit patterns) IN HBM; fp32 accumulation; one v_mfma_f32_32x32x16_bf16 per product.
 *   vqcpc_cast_bf16      out[r][c] = bf16_rne(in[r * ld_in + c])  (what torch's .bfloat16() does), dense [rows][cols]
 *   vqcpc_gemm_nt_bf16   C / Cb = epilogue(A[M,K] . B[N,K]^T): replaces F.linear on bf16-cast operands
 *                        (transformer_custom.py:282-289 FFN, multihead_attention_custom.py:171-196,338 projections).
 *                        C (fp32) and / or Cb (bf16) receive the result; epilogue as vqcpc_gemm_nt (bias, act = 1 relu,
 *                        dropout, gate: out *= gate > 0 ? gate_scale : 0 with an fp32 `gate` or a bf16 `gate_bf16` operand,
 *                        add: an fp32 `add` or -- round 5, the residual stream of the bf16 path kept in bf16: the LayerNorm's
 *                        bf16 output is then its ONLY output -- a bf16 `add_bf16` operand, bias / bias + dropout epilogues; the
 *                        residual sum may itself leave as Cb only: vqcpc_layernorm_fwd_xb16 / _bwd_xb16 read it so).
 *                        M, N multiples of 256, K of 64 (vqcpc_gemm_nt_bf16_supported); lda / ldb / ldcb / ldgate_bf16 /
 *                        ldadd_bf16 in bf16 elements.
 *   vqcpc_gemm_tn_bf16   dW[N,K] (+)= A[M,N]^T . B[M,K], db[N] (+)= column sums of A: the weight / bias gradient of F.linear
 *                        on bf16 operands (what autograd derives for the calls above); as vqcpc_gemm_tn.  M multiple of 128,
 *                        N and K of 256 (vqcpc_gemm_tn_bf16_supported).
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_cast_bf16(const float* in, int64_t ld_in, void* out, int64_t rows, int cols, void* stream);
int vqcpc_gemm_nt_bf16_supported(int64_t M, int N, int K);
/* vqcpc_gemm_nt_bf16 / vqcpc_gemm_tn_bf16 deliver their operands global -> LDS by DMA in whole 128-byte lines -- NT: K tiles of
 * 64, one barrier per K tile (K % 128 == 0, otherwise the register-staged ping-pong kernel with K tiles of 32: bit-identical
 * results); TN: 64-row slots in their row-major form, fragments by ds_read_b64_tr_b16. */
int vqcpc_gemm_nt_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, void* Cb, int64_t ldcb,
                       int64_t M, int N, int K, const float* bias, int act, float drop_p, uint64_t seed, const float* gate,
                       int64_t ldgate, const void* gate_bf16, int64_t ldgate_bf16, float gate_scale, const float* add,
                       int64_t ldadd, const void* add_bf16, int64_t ldadd_bf16, void* stream);
int vqcpc_gemm_tn_bf16_supported(int64_t M, int N, int K);
int64_t vqcpc_gemm_tn_bf16_workspace(int64_t M, int N, int K);
int vqcpc_gemm_tn_bf16(const void* A, int64_t lda, const void* B, int64_t ldb, float* dW, float* db, int64_t M, int N, int K,
                       int accumulate, void* workspace, int64_t workspace_bytes, void* stream);

/* dst[i][0 .. counts[i]) += src[i][..] for up to 8 small tensors in one launch (host arrays of device pointers): the
 * `param.grad += g` of the small per-layer parameters (LayerNorm gamma / beta, relative-position tables) that autograd's
 * AccumulateGrad would run as one kernel each (transformer_custom.py:282-289, subsampled_relative_attention.py:23-26). */
int vqcpc_accumulate8(float* const* dst, const float* const* src, const int* counts, int n_tensors, void* stream);

/* Number of distinct merged product codes (sum_c idx[c] K^c) among the rows of up to two (rows, num_codebooks) int64 index
 * tensors -> out[0] (as float): the `num_codewords` / `num_codewords_negative` metrics of VQCPCEncoderTrainer.epoch
 * (vqcpc_encoder_trainer.py:320-331, len(torch.unique(.))) without a sort and without a host sync.  One bit per possible
 * code in LDS: `_supported` is 0 when codebook_size ^ num_codebooks exceeds 2^20 (the caller counts with a sort then). */
int vqcpc_count_distinct_codes_supported(int num_codebooks, int codebook_size);
int vqcpc_count_distinct_codes(const int64_t* idx_a, int64_t rows_a, const int64_t* idx_b, int64_t rows_b, int num_codebooks,
                               int codebook_size, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * relu / dropout gate of the feed-forward block as a bit mask (transformer_custom.py:285: linear2(dropout(relu(linear1(x))))).
 *   vqcpc_gemm_nt_relu_mask   C = dropout(relu(A . B^T + bias)) as vqcpc_gemm_nt(act = 1, drop_p, seed), and one bit per
 *                             element "C > 0" into `mask` (vqcpc_gemm_gatebits_bytes(M, N) bytes; word
 *                             ((row >> 2) * N/32 + col/32) * 4 + (row & 3), bit col % 32)
 *   vqcpc_gemm_nt_gatebits    C = (A . B^T) * (bit ? gate_scale : 0): the backward of relu + dropout folded into the dgrad
 *                             GEMM as with vqcpc_gemm_nt(gate = activation), reading 1/32 of the bytes
 *   bf16x6 mode, M and N multiples of 256, K of 32 (vqcpc_gemm_gatebits_supported); same numbers as the fp32-gate calls.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_gemm_gatebits_supported(int64_t M, int N, int K);
int64_t vqcpc_gemm_gatebits_bytes(int64_t M, int N);
int vqcpc_gemm_nt_relu_mask(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N,
                            int K, const float* bias, float drop_p, uint64_t seed, void* mask, void* stream);
int vqcpc_gemm_nt_gatebits(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N,
                           int K, const void* mask, float gate_scale, void* stream);

/* Split-K form of vqcpc_gemm_nt for launches that cannot fill the chip (few 128 x 128 tiles, long K: the d_model-wide
 * projections of the student step, encoder_student_trainer.py:203-262 -> transformer_custom.py:270-295 at 3072 / 768 rows).
 *   vqcpc_gemm_nt_splitk_workspace   bytes of partial-sum workspace, or 0 when (M, N, K) is not a split-K shape in the
 *                                    current GEMM mode (then call vqcpc_gemm_nt).
 *   vqcpc_gemm_nt_splitk             C = A . B^T (+ bias) (+ add); the K range is cut into partial planes in `workspace`,
 *                                    summed in a fixed order (deterministic).  Epilogues other than bias / add: vqcpc_gemm_nt. */
int64_t vqcpc_gemm_nt_splitk_workspace(int64_t M, int N, int K);
/* rows of an (M, N, K) product that vqcpc_gemm_nt hands to whole rounds of its 256-tile kernel when it cuts the launch by rows
 * (M when it does not): the caller may run rows [main, M) through vqcpc_gemm_nt_splitk and rows [0, main) through vqcpc_gemm_nt */
int64_t vqcpc_gemm_nt_main_rows(int64_t M, int N, int K);
int vqcpc_gemm_nt_splitk(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int N,
                         int K, const float* bias, const float* add, int64_t ldadd, void* workspace, int64_t workspace_bytes,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Whole-step HIP-graph replay (vqcpc_bach_amd/graphs.py).  A captured step freezes its kernel ARGUMENTS, so the values
 * that must change every step live on the device:
 *   - dropout: every seed is XOR-ed with a step salt (0 outside graph replay).  vqcpc_rng_salt_advance is the first node
 *     of a captured step: counter[0] += 1, salt = splitmix64(base ^ counter[0]); vqcpc_rng_salt_set writes it directly
 *     (value 0 restores eager behaviour).  This is the ONE piece of library state: a process-wide device value.
 *   - Adam (vqcpc_adam_step_dev = vqcpc_adam_step with lr read from lr_dev[0] and the step count t -- the bias
 *     corrections 1 - beta^t -- from step_dev[0], the counter that vqcpc_rng_salt_advance increments).
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_rng_salt_set(uint64_t value, void* stream);
int vqcpc_rng_salt_advance(uint64_t* counter, uint64_t base, void* stream);
/* the salt of the CURRENT counter value again, without advancing it: first node of a later captured stage of the same step
 * (a step cut into several graphs around eagerly issued, bucketed all-reduces) */
int vqcpc_rng_salt_from_counter(const uint64_t* counter, uint64_t base, void* stream);
int vqcpc_adam_step_dev(float* p, float* g, float* m, float* v, int64_t n, const float* lr_dev, float beta1, float beta2,
                        float eps, const uint64_t* step_dev, float grad_scale, float max_norm, const double* sumsq,
                        void* stream);

/* Weight averaging (opt-in: FlatTraining.enable_weight_averaging): an exponential moving average of the flat parameters, one
 * launch after Adam's, in place on avg [n]:
 *       d_u = min(decay, float(1 + u) / float(10 + u)) ;  w = 1 - d_u ;  avg[i] = avg[i] + w * (p[i] - avg[i])
 *   all fp32, every operation rounded on its own (no FMA): a numpy float32 restatement gives the same bits.
 *   u = the number of averaging updates so far, counting this one.  Host form: step_dev NULL, u >= 1 an argument.  Device
 *   form (a captured step): u = step_dev[0] - t0, step_dev the counter vqcpc_adam_step_dev reads as Adam's t and t0 Adam's
 *   step count when averaging was enabled; step_dev[0] <= t0 leaves avg untouched.
 *   avg and p need only be 4-byte aligned (float4 accesses are used where both permit them); no element at an index >= n
 *   is read or written.  Refused before any HIP call: null avg or p, n < 0, decay outside [0, 1), the host form with
 *   u < 1.  n == 0 launches nothing. */
int vqcpc_weight_average(float* avg, const float* p, int64_t n, float decay, uint64_t u, const uint64_t* step_dev, uint64_t t0,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Autoregressive generation (VQCPCB/decoders/decoder.py:552-723, utils.py:101-128): the kernels of one KV-cached
 * decoder step for M <= 64 sequences (vqcpc_bach_amd/decoders/generation.py).  Adding them left the ABI version alone.
 *
 * vqcpc_decode_linear: y[M][N] = relu?(x W^T + bias) + res  (bias, res optional; relu != 0 applies the ReLU before the
 *   residual).  x row m = x + (gather ? gather[m] : m) * ldx; W [N][K] row-major.  M <= 64, N, K <= 4096, K % 4 == 0.
 *   Plain fp32 FMA in a fixed reduction order per element that does not depend on M (batch-invariant rows).  y != x.
 * vqcpc_decode_attn: one query row per (sequence b, head h); the position is read from pos[0] (device int32).
 *   Self mode (k_new, v_new != NULL; mask 1, ratio 1): rows b of k_new / v_new (stride ldn, head h = columns [h*hd,
 *   (h+1)*hd)) are stored into k_cache / v_cache at row b * Lk + pos (stride ldc), then keys 0..pos are attended with the
 *   bias q.e1[h, Lk-1-(pos-j)].  Cross mode (k_new == NULL): the Lk cached memory rows, p = pos / ratio, mask 0 none /
 *   1 causal (j <= p) / 2 anticausal (j >= p), bias of vqcpc_relattn_x_fwd.  q unscaled; ctx [M][ldo].  hd in
 *   {16, 32, 64, 128}, Lk <= 1024, no dropout.
 * vqcpc_decode_attn_probs: vqcpc_decode_attn (the same kernel body, a compile-time flag; ctx and the cache rows have the same
 *   bits) which also writes the row of attention probabilities it multiplies V by: probs is [M][H][rows][ldp] float32,
 *   ldp >= Lk, and a live launch (0 <= pos, p < Lk) writes probs[b][h][r][j] for every j in [0, Lk) at row r = pos (win ==
 *   NULL) or r = win[1] * win_stride + pos -- the rule of vqcpc_decode_sample_constrained's column, so with win_stride = U the
 *   rows are chorale positions and one captured step serves every window.  The value is exp(s_j - max) / sum as the kernel
 *   holds it, +0.0f for a masked key and, in self mode, for j > pos.  Columns [Lk, ldp) and every other row are never
 *   touched.  With r outside [0, rows), or no live window (win[1] < 0), no probability is written and ctx and the cache rows
 *   are still produced; a dead launch writes nothing at all.  rows >= 1; win_stride >= 1 when win is given.
 * vqcpc_decode_sample: one step's tail, ONE workgroup.  voice c = pos % nc; voice_offsets (HOST int32 [nc + 1]) give its
 *   logits columns.  Per row b: logits / temperature, tokens whose bit is set in exclude[c][8] (device uint32, NULL =
 *   none) to -inf, top-k (drop logits < the k-th largest; 0 = off), top-p (utils.py:116-126; top_p <= 0 or >= 1 = off),
 *   softmax, one draw from the counter-based hash keyed by (seeds[b], pos) -- or, teacher != NULL, the token
 *   teacher[b * ldteach + pos].  Writes tokens[b * ldtok + pos], next_in row b = table row token * U + pos % U (the
 *   input of position pos + 1, decoders/decoder.py:_target_rows), optionally the filtered probabilities probs[b][0..V_c),
 *   and finally pos[0] = pos + 1.  Nothing happens once pos >= T.  M <= 64, nc <= 16, V_c <= 256, d <= 4096.
 * vqcpc_decode_sample_constrained: vqcpc_decode_sample (the same kernel body, a compile-time flag) without teacher, with
 *   seeds required, and three more things, all addressed at column col = pos (win == NULL) or win[1] * U + pos -- win[1]
 *   (device int32) is the live window's first code as vqcpc_decode_window leaves it, the rule of vqcpc_decode_source_rows,
 *   so constraint and logp are in chorale coordinates and one captured step or slide serves every window:
 *     constraint[b * ldcons + col] (device int64, NULL = nothing forced): >= 0 is the token to emit, clamped to [0, V_c)
 *       as teacher is; < 0 draws the token exactly as vqcpc_decode_sample does, keyed by (seeds[b], pos) -- forcing some
 *       positions does not shift the draws of the others.  A forced token ignores exclude / top-k / top-p.
 *     logp[b * ldlogp + col] (may be NULL) = logits[tok] - logsumexp(logits) over the voice's V_c columns for the emitted
 *       token, forced or drawn: the model's UNMODIFIED distribution (temperature 1, no filter).  fp32, the maximum
 *       subtracted, summed in an order that depends on the lane layout only (a row's value does not depend on M).
 *     win[1] < 0: nothing is forced and no logp is written.  Likewise for a column col >= ldcons (free) / col >= ldlogp
 *       (not written): the window index is not known to the host, which checks ldcons, ldlogp >= T only.
 *   probs, next_in, tokens[b * ldtok + pos], pos[0] = pos + 1, the no-op once pos >= T and the limits are unchanged.
 * vqcpc_decode_sample_masked: vqcpc_decode_sample_constrained (the same kernel body, one more compile-time flag) with two more
 *   things at the same column col:
 *     allowed[(b * ldallow + col) * 8 + w] (device uint32, [M][ldallow][8]; NULL = no restriction): bit i & 31 of word i >> 5
 *       set means token i may be drawn at (row b, column col).  A token outside the set becomes -inf where exclude is applied
 *       (after / temperature, before top-k and top-p), so the filters and probs act on the allowed set; the draw is still
 *       keyed by (seeds[b], pos).  Only bits [0, V_c) count; a set with none of them restricts nothing (the caller is expected
 *       to refuse such a set).  A forced token (constraint >= 0) wins over the set as it wins over exclude.  col >= ldallow or
 *       win[1] < 0: no restriction.
 *     logmass[b * ldmass + col] (may be NULL; column rule of logp) = (m_a - m) + log(s_a) - log(s): m, s the maximum and the
 *       exp-sum of the unmodified row as logp forms them, m_a, s_a the same over the allowed tokens, summed in the same lane
 *       order -- the log of the probability the model itself gives to the allowed set (temperature 1, no filter, exclude not
 *       counted).  Exactly 0.0f for the full set and for a row that is not restricted, -inf when every allowed logit is -inf;
 *       written at forced positions too; a row's value does not depend on M.  logp is unchanged: the emitted token under the
 *       unmodified row.
 *   ldallow >= T with allowed, ldmass >= T with logmass.  With allowed == NULL and logmass == NULL every output has the bits of
 *   vqcpc_decode_sample_constrained.
 *
 * Sliding-window generation (decoders/decoder.py:729-854): the window moves by one code, the caches of its P prefix rows
 * are rebuilt teacher-forced (vqcpc_gemm_nt, vqcpc_add_layernorm_fwd, vqcpc_block_table_gather for the row-wise parts).
 * vqcpc_decode_prefill_attn: query rows i in [0, P) of each of M sequences, q row b * P + i (stride ldq), at position i
 *   of an Lq = ratio * Lk problem whose tables e1, e2 have Lk rows.  Self mode (k_cache, v_cache != NULL; mask 1, ratio 1):
 *   k / v rows b * P + j (stride ldk; the in_proj output) are stored into k_cache / v_cache at row b * Lk + j (stride ldc),
 *   keys 0..i are attended with the bias q.e1[h, Lk-1-(i-j)]; ctx == NULL stores the rows and stops.  Cross mode
 *   (k_cache == NULL): k / v rows b * Lk + j of the memory, p = i / ratio, masks and bias as vqcpc_decode_attn's cross
 *   mode.  ctx row b * P + i (stride ldo).  Tiled (16 query rows per workgroup, K / V / table tiles in LDS, masked key
 *   tiles skipped), online fp32 softmax, no probabilities written, no dropout.  hd in {16, 32, 64, 128}.
 * vqcpc_decode_window: ONE workgroup; win (device int32 [2]) = {next window's first code, live window's first code or
 *   -1}.  First the live window's tokens [0, pos) go back into chorale[M][ldch] (token t of window w is chorale column
 *   w * U + t).  Then, unless win[0] < 0 or win[0] + S > nb (commit only): codes_win[M][S] = codes_full[M][nb] columns
 *   win[0].., tokens[M][T] = the chorale's columns win[0] * U.., prefix_rows[b * P + j] = the table row of input j
 *   (start-of-sentence row table_rows - 1 at j = 0, else token[j-1] * U + (j-1) % U), x row b = the input row of position
 *   P, seeds_out[b] = seeds_in[b] for window 0, otherwise splitmix64(seeds_in[b] ^ win[0] * 0xD1B54A32D192ED03) -- the
 *   sampler keys its draw by (seed, window position), so the seed must change with the window --, pos[0] = P,
 *   win = {win[0] + advance, win[0]}.  T == S * U, 0 <= P < T.
 * vqcpc_decode_source_rows: the source rows of a decoder on CONTINUOUS latents (a NoQuantization encoder; decoder.py:222-229
 *   makes source_embeddings an nn.Linear(dz, d_model)): for b < M, j < S, n < N
 *     src[(b * S + j) * lds + n] = bias[n] + sum_k z_full[(b * nb + w0 + j) * dz + k] * w[n * dz + k],
 *   w0 = win ? win[1] : 0 -- the live window's first code as vqcpc_decode_window leaves it, read from device memory, so a
 *   captured slide serves every middle window.  Nothing is written if w0 < 0 or w0 + S > nb.  Plain fp32 FMA, k ascending
 *   from 0, the bias added last: a row's result depends on its own latents and W only (not on M, b, w0 or other rows).
 *   bias may be NULL.  M <= 64, S <= 1024, 4 <= dz <= 256, dz % 4 == 0, N <= 4096, lds >= N, nb >= S.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_decode_linear(const float* x, int64_t ldx, const int64_t* gather, const float* w, const float* bias, const float* res,
                        int64_t ldr, float* y, int64_t ldy, int64_t M, int N, int K, int relu, void* stream);
int vqcpc_decode_attn(const float* q, int64_t ldq, float* k_cache, float* v_cache, int64_t ldc, const float* k_new,
                      const float* v_new, int64_t ldn, const float* e1, const float* e2, float* ctx, int64_t ldo,
                      const int32_t* pos, int64_t M, int Lk, int ratio, int H, int hd, int mask, void* stream);
int vqcpc_decode_attn_probs(const float* q, int64_t ldq, float* k_cache, float* v_cache, int64_t ldc, const float* k_new,
                            const float* v_new, int64_t ldn, const float* e1, const float* e2, float* ctx, int64_t ldo,
                            const int32_t* pos, int64_t M, int Lk, int ratio, int H, int hd, int mask, float* probs, int64_t ldp,
                            int64_t rows, const int32_t* win, int win_stride, void* stream);
int vqcpc_decode_sample(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M, float temperature,
                        int top_k, float top_p, const uint32_t* exclude, const int64_t* seeds, const int64_t* teacher,
                        int64_t ldteach, int64_t* tokens, int64_t ldtok, int T, const float* table, int64_t table_rows, int d,
                        int U, float* next_in, int64_t ldn, float* probs, int64_t ldp, int32_t* pos, void* stream);
int vqcpc_decode_sample_constrained(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M,
                                    float temperature, int top_k, float top_p, const uint32_t* exclude, const int64_t* seeds,
                                    const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win,
                                    int64_t* tokens, int64_t ldtok, int T, const float* table, int64_t table_rows, int d, int U,
                                    float* next_in, int64_t ldn, float* probs, int64_t ldp, int32_t* pos, void* stream);
int vqcpc_decode_sample_masked(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M, float temperature,
                               int top_k, float top_p, const uint32_t* exclude, const int64_t* seeds, const int64_t* constraint,
                               int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win, const uint32_t* allowed,
                               int64_t ldallow, float* logmass, int64_t ldmass, int64_t* tokens, int64_t ldtok, int T,
                               const float* table, int64_t table_rows, int d, int U, float* next_in, int64_t ldn, float* probs,
                               int64_t ldp, int32_t* pos, void* stream);
int vqcpc_decode_prefill_attn(const float* q, int64_t ldq, const float* k, const float* v, int64_t ldk, float* k_cache,
                              float* v_cache, int64_t ldc, const float* e1, const float* e2, float* ctx, int64_t ldo, int64_t M,
                              int P, int Lk, int ratio, int H, int hd, int mask, void* stream);
int vqcpc_decode_window(const int64_t* codes_full, int64_t nb, int64_t* chorale, int64_t ldch, int32_t* win, int advance,
                        int64_t* codes_win, int S, int64_t* tokens, int T, int U, int P, int64_t* prefix_rows,
                        const float* table, int64_t table_rows, int d, float* x, int64_t ldx, const int64_t* seeds_in,
                        int64_t* seeds_out, int32_t* pos, int64_t M, void* stream);
int vqcpc_decode_source_rows(const float* z_full, int64_t nb, int dz, const int32_t* win, const float* w, const float* bias,
                             float* src, int64_t lds, int64_t M, int S, int N, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Sampling code sequences from the prior (VQCPCB/priors/prior_relative.py:308-353: one full forward per code, softmax,
 * p ** temperature renormalised, np.random.choice on the host).  The prior's KV-cached step is made of vqcpc_decode_linear,
 * vqcpc_decode_attn (self mode), vqcpc_add_layernorm_fwd and, for the re-prefill of a moved window, vqcpc_gemm_nt and
 * vqcpc_decode_prefill_attn (vqcpc_bach_amd/priors/generation.py); the two entry points below are its tail and its window
 * bookkeeping (csrc/prior.hip).  Adding them left the ABI version alone.
 *
 * vqcpc_prior_sample: one workgroup per row b < M <= 64, V <= 4096 codes.  The position is read from pos[0] (device
 *   int32); nothing happens once pos >= N.  Per row: logits[b][0..V) * temperature -- the reference's sense (:346,
 *   p ** temperature renormalised == softmax(temperature * logits)), the OPPOSITE of vqcpc_decode_sample's division --,
 *   top-k (drop logits < the k-th largest; 0 = off), top-p (utils.py:116-126; top_p <= 0 or >= 1 = off), softmax, one draw
 *   from the counter-based hash keyed by (seeds[b], pos) -- or, teacher != NULL, the code teacher[b * ldteach + pos].
 *   Writes codes[b * ldc + pos], next_in row b = table row `code` (the input of position pos + 1; table [table_rows][d],
 *   table_rows >= V), optionally the filtered probabilities probs[b][0..V).  The last workgroup to finish (ticket: device
 *   int32, zero before the first call, zero again after every call) writes pos[0] = pos + 1.  Every reduction runs inside
 *   the row's workgroup in an order that depends on V only: a row's codes do not depend on M.
 * vqcpc_prior_sample_constrained: vqcpc_prior_sample (the same kernel body, a compile-time flag) without teacher, with seeds
 *   required, and three more things, all addressed at the sequence column col = pos (win == NULL) or win[1] + pos -- win[1]
 *   (device int32) is the live window's first code as vqcpc_prior_window leaves it, code j of window w being sequence column
 *   w + j, so constraint and logp are in sequence coordinates and one captured step and one captured move serve every window:
 *     constraint[b * ldcons + col] (device int64, NULL = nothing forced): >= 0 is the code to emit, clamped to [0, V) as
 *       teacher is; < 0 draws the code exactly as vqcpc_prior_sample does, keyed by (seeds[b], pos) -- forcing some positions
 *       does not shift the draws of the others.  A forced code ignores top-k / top-p.
 *     logp[b * ldlogp + col] (may be NULL) = logits[code] - logsumexp(logits[0..V)) for the emitted code, forced or drawn: the
 *       model's UNMODIFIED distribution (temperature 1, no filter).  fp32, the maximum subtracted, reduced inside the row's
 *       workgroup in an order that depends on V only (a row's value does not depend on M).  -inf logits contribute zero; a
 *       forced code whose logit is -inf gets -inf.
 *     win[1] < 0: nothing is forced and no logp is written.  Likewise for a column col >= ldcons (free) / col >= ldlogp
 *       (not written): the window index is not known to the host, which checks ldcons, ldlogp >= N only.
 *   codes[b * ldc + pos], next_in, probs (the filtered distribution whatever is forced), the ticket that advances pos[0], the
 *   no-op once pos >= N and the limits are unchanged.
 * vqcpc_prior_sample_masked: vqcpc_prior_sample_constrained (the same kernel body, one more compile-time flag) with two more
 *   things at the same column col (col = pos, or win[1] + pos; win[1] < 0: no live window):
 *     allowed[(b * ldallow + col) * words + w] (device uint32, [M][ldallow][words], words = ceil(V / 32) <= 128; NULL = no
 *       restriction): bit i & 31 of word i >> 5 set means code i may be drawn at (row b, column col).  A code outside the set
 *       becomes -inf right after logits * temperature, before top-k and top-p, so the filters and probs act on the allowed codes;
 *       the draw is still keyed by (seeds[b], pos).  Thread t reads the one word that holds its 16 codes.  Only bits [0, V) count;
 *       a set with none of them restricts nothing (the caller is expected to refuse such a set).  A forced code (constraint >= 0)
 *       wins over the set.  col outside [0, ldallow) or no live window: no restriction.
 *     logmass[b * ldmass + col] (may be NULL; column rule of logp) = (m_a - m) + log(s_a) - log(s): m, s the maximum and the
 *       exp-sum of the unmodified row exactly as logp forms them (a thread's 16 codes ascending, then the block sum), m_a, s_a the
 *       same over the allowed codes in the same order -- the log of the probability the model itself gives to the set
 *       (temperature 1, no filter).  Exactly 0.0f for the full set and for a row that is not restricted, -inf when every allowed
 *       logit is -inf; written at forced columns too; a row's value does not depend on M.  logp is unchanged: the emitted code
 *       under the unmodified row.
 *   ldallow >= N with allowed, ldmass >= N with logmass.  With allowed == NULL and logmass == NULL every output has the bits of
 *   vqcpc_prior_sample_constrained.
 * vqcpc_prior_window: ONE workgroup; win (device int32 [2]) = {next window's first code, live window's first code or -1}.
 *   First the live window's codes [0, pos) go back into seq[M][ldseq] (code j of window w is column w + j).  Then, unless
 *   win[0] < 0 or win[0] + N > num_tokens (commit only): codes_win[M][N] = seq columns win[0].., prefix_rows[b * P + j] =
 *   the table row of input j (start-of-sentence row table_rows - 1 at j = 0, else code j - 1 of the window), x row b = the
 *   input row of position P, seeds_out[b] by the rule of vqcpc_decode_window, pos[0] = P, win = {win[0] + advance, win[0]}.
 *   0 <= P < N <= 1024.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_prior_sample(const float* logits, int64_t ldl, int V, int64_t M, float temperature, int top_k, float top_p,
                       const int64_t* seeds, const int64_t* teacher, int64_t ldteach, int64_t* codes, int64_t ldc, int N,
                       const float* table, int64_t table_rows, int d, float* next_in, int64_t ldn, float* probs, int64_t ldp,
                       int32_t* pos, int32_t* ticket, void* stream);
int vqcpc_prior_sample_constrained(const float* logits, int64_t ldl, int V, int64_t M, float temperature, int top_k, float top_p,
                                   const int64_t* seeds, const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp,
                                   const int32_t* win, int64_t* codes, int64_t ldc, int N, const float* table,
                                   int64_t table_rows, int d, float* next_in, int64_t ldn, float* probs, int64_t ldp,
                                   int32_t* pos, int32_t* ticket, void* stream);
int vqcpc_prior_sample_masked(const float* logits, int64_t ldl, int V, int64_t M, float temperature, int top_k, float top_p,
                              const int64_t* seeds, const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp,
                              const int32_t* win, const uint32_t* allowed, int64_t ldallow, float* logmass, int64_t ldmass,
                              int64_t* codes, int64_t ldc, int N, const float* table, int64_t table_rows, int d, float* next_in,
                              int64_t ldn, float* probs, int64_t ldp, int32_t* pos, int32_t* ticket, void* stream);
int vqcpc_prior_window(int64_t* seq, int64_t ldseq, int64_t num_tokens, int32_t* win, int advance, int64_t* codes_win, int N,
                       int P, int64_t* prefix_rows, const float* table, int64_t table_rows, int d, float* x, int64_t ldx,
                       const int64_t* seeds_in, int64_t* seeds_out, int32_t* pos, int64_t M, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The prior over PRODUCT codes (prior_kwargs['code_model'] = 'product'; csrc/product_codes.hip, the kernel bodies of the three
 * entry points above under a compile-time flag).  A code is predicted digit by digit: a step's tail is, per stage j = 0 ..
 * ncb - 1, one vqcpc_decode_linear (head j on h_j) and one vqcpc_prior_sample_product.  Notation and limits of the "Product
 * codes" section: digit j of a code is (code / K^j) % K, V = K^ncb.  Adding them left the ABI version alone.
 *
 * vqcpc_prior_sample_product: ONE STAGE.  One workgroup per row b < M <= 64; nothing happens at any stage once pos[0] >= N.
 *   logits[b][0..K) are the stage's.  Temperature (multiplication, the prior's sense), top-k and top-p filter THIS stage's
 *   distribution exactly as vqcpc_prior_sample filters a row of K codes; probs[b][0..K) (may be NULL) receives it.
 *   The digit: digit `stage` of teacher[b * ldteach + pos] (teacher != NULL; negative codes count as 0), else digit `stage` of
 *   constraint[b * ldcons + col] where that is >= 0 -- a forced code is clamped to [0, V) first --, col = pos (win == NULL) or
 *   win[1] + pos and the win[1] < 0 / col >= ldcons rules of vqcpc_prior_sample_constrained; else ONE draw from the stage's
 *   filtered distribution.  A forced digit ignores the filters; a free one is drawn as if nothing were forced.
 *   Draw keys: stage 0 draws with (seeds[b], pos), the merged sampler's key; stage j >= 1 with (s_j, pos),
 *     s_j = splitmix64(seeds[b] XOR j * 0xA0761D6478BD642F)   (splitmix64: the finaliser vqcpc_decode_window's seed rule uses).
 *   No key depends on M.  With ncb = 1 the kernel is vqcpc_prior_sample_constrained bit for bit (and so vqcpc_prior_sample,
 *   where nothing is forced and logp == NULL): codes, next_in, probs, logp, pos, ticket.
 *   Stage log-probability (computed when logp != NULL and col is in [0, ldlogp) with win[1] >= 0):
 *     logits[digit] - logsumexp(logits[0..K)), unfiltered, temperature 1, reduced in an order that depends on K only; stage 0
 *     STORES it in logp_acc[b], stage j >= 1 ADDS it (logp_acc[b] + own, one fp32 add, ascending j).
 *   A stage j < ncb - 1 then stores its digit in digits[b * ncb + j] (device int32 scratch [M][ncb]) and writes
 *     h_next[b][:] = h[b][:] + dtab[j][digit][:]   (one fp32 add per element; dtab [ncb - 1][K][d], the prior's digit-conditioning
 *     table; h [M][ldh] is what this stage's head read, h_next [M][ldhn] what the next stage's head reads)
 *   and touches neither codes, next_in, logp, pos nor the ticket.  The LAST stage forms the merged code from digits[b][0 ..
 *   ncb - 1) and its own digit, writes codes[b * ldc + pos], next_in row b = tables[0][c_0] + tables[1][c_1] + ... (tables
 *   [ncb][K][d]: the chain of vqcpc_product_gather without res, same order, same bits), logp[b * ldlogp + col] = the accumulated
 *   sum, and advances pos[0] through the ticket as vqcpc_prior_sample does.
 * vqcpc_prior_sample_product_masked: vqcpc_prior_sample_product with what vqcpc_prior_sample_masked adds, per stage.  The set of
 *   stage j at (row b, column col) is the words = ceil(K / 32) words at allowed[((b * ldallow + col) * ncb + j) * words] (device
 *   uint32, [M][ldallow][ncb][words]): a product code's allowed set is the Cartesian product of its digit sets, the one form that
 *   needs no array of K^ncb entries.  A digit outside its set becomes -inf before the stage's filters; only bits [0, K) count, a
 *   digit set with none of them restricts nothing; a forced digit (teacher excludes the mask; constraint >= 0) wins.
 *   Stage log-mass (computed when logmass != NULL and col is in [0, ldmass) with a live window): (m_a - m) + log(s_a) - log(s) of
 *   the stage's row and set as in vqcpc_prior_sample_masked; stage 0 STORES it in mass_acc[b] (device float scratch [M]), stage
 *   j >= 1 ADDS it (one fp32 add, ascending j), the last stage writes the sum to logmass[b * ldmass + col].  That number is the sum
 *   of the per-digit conditional masses ALONG THE EMITTED DIGITS -- the incremental importance weight of the digit-by-digit
 *   proposal --, NOT the marginal mass of the product set under the model.  logp is unchanged.  With ncb = 1 the kernel is
 *   vqcpc_prior_sample_masked bit for bit; with allowed == NULL and logmass == NULL, vqcpc_prior_sample_product.
 * vqcpc_prior_window_product: vqcpc_prior_window (commit, load, seeds rule, pos = P, win update) with the product row rule:
 *   prefix_rows[b * P + j] = the merged code of input j clamped to [0, V), or V for the start-of-sentence input (j = 0); x row b
 *   = the vqcpc_product_gather chain over tables [ncb][K][d] of the input of position P, or sos [d] when P = 0.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_prior_sample_product(const float* logits, int64_t ldl, int K, int ncb, int stage, int64_t M, float temperature, int top_k,
                               float top_p, const int64_t* seeds, const int64_t* teacher, int64_t ldteach,
                               const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win,
                               int32_t* digits, float* logp_acc, const float* h, int64_t ldh, const float* dtab, float* h_next,
                               int64_t ldhn, int64_t* codes, int64_t ldc, int N, const float* tables, int d, float* next_in,
                               int64_t ldn, float* probs, int64_t ldp, int32_t* pos, int32_t* ticket, void* stream);
int vqcpc_prior_sample_product_masked(const float* logits, int64_t ldl, int K, int ncb, int stage, int64_t M, float temperature,
                                      int top_k, float top_p, const int64_t* seeds, const int64_t* teacher, int64_t ldteach,
                                      const int64_t* constraint, int64_t ldcons, float* logp, int64_t ldlogp, const int32_t* win,
                                      const uint32_t* allowed, int64_t ldallow, float* logmass, int64_t ldmass, int32_t* digits,
                                      float* logp_acc, float* mass_acc, const float* h, int64_t ldh, const float* dtab,
                                      float* h_next, int64_t ldhn, int64_t* codes, int64_t ldc, int N, const float* tables, int d,
                                      float* next_in, int64_t ldn, float* probs, int64_t ldp, int32_t* pos, int32_t* ticket,
                                      void* stream);
int vqcpc_prior_window_product(int64_t* seq, int64_t ldseq, int64_t num_tokens, int32_t* win, int advance, int64_t* codes_win,
                               int N, int P, int64_t* prefix_rows, const float* tables, int ncb, int K, const float* sos, int d,
                               float* x, int64_t ldx, const int64_t* seeds_in, int64_t* seeds_out, int32_t* pos, int64_t M,
                               void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The aligned ("diagonal") cross block of the decoder (TransformerAlignedDecoderLayerCustom,
 * VQCPCB/transformer/transformer_custom.py:389-492; csrc/aligned.hip).  C = cross_attn(memory rows) is [n * S][nc * d] with
 * feature index j * nc + v (feature j of voice v, the reshape of :476); a code covers U = epc * nc target tokens
 * t = event * nc + voice.  fp32, no atomics, fixed summation order, graph-capture safe.  Adding them left the ABI version
 * alone.  nc * d <= 16384, U % nc == 0.
 *
 * vqcpc_aligned_expand (:476-481, reshape / permute / repeat_interleave / reshape): out [n * P][d], row b * P + i =
 *   C[b * S + i / U][(.) * nc + i % nc]; P <= S * U rows per sequence (a trailing partial code is written in part).
 * vqcpc_aligned_reduce (the backward of the above for P = S * U): d_C[b * S + s][j * nc + v] =
 *   sum_{e < epc} d_out[b * S * U + (s * epc + e) * nc + v][j], e ascending.
 * vqcpc_elu_fwd / vqcpc_elu_bwd (nn.ELU of cross_attn, :428, alpha = 1): y = x > 0 ? x : expm1(x);
 *   g_x = x > 0 ? g_out : g_out * exp(x), x the PRE-activation.  expm1 / exp in double, one rounding.
 * vqcpc_decode_aligned_add (:475-482 at one position, eval mode): s[b][j] = h[b][j] + C[b * S + pos / U][j * nc + pos % nc],
 *   pos read from pos[0] (device int32) as the kernels of the generation step do; nothing happens unless
 *   0 <= pos < S * U.  M <= 64 rows.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_aligned_expand(const float* C, float* out, int64_t n, int S, int P, int U, int nc, int d, void* stream);
int vqcpc_aligned_reduce(const float* d_out, float* d_C, int64_t n, int S, int U, int nc, int d, void* stream);
int vqcpc_elu_fwd(const float* x, float* y, int64_t n, void* stream);
int vqcpc_elu_bwd(const float* x, const float* g_out, float* g_x, int64_t n, void* stream);
int vqcpc_decode_aligned_add(const float* h, int64_t ldh, const float* C, float* s, int64_t lds, const int32_t* pos, int64_t M,
                             int S, int U, int nc, int d, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Device-resident window sampler over a tokenised corpus (csrc/corpus.hip, vqcpc_bach_amd/dataloaders/corpus.py; the window
 * rule restates VQCPCB/datasets/chorale_dataset.py:124-129, 418-470).  Device tables: tokens (total_ticks, 4) int32, 16-byte
 * aligned, the pieces concatenated; piece_start (P + 1) tick offsets; special = START[4] END[4] PAD[4]; win_cum (P + 1), the
 * cumulative window counts of ONE window length W (beats of `subdivision` ticks): piece p has last[p] + W windows, start beats
 * o = -(W - 1) .. last[p], 0 <= last[p] <= beats(p) - 1.
 * vqcpc_corpus_permute: ids[i] = lo + pi_key((q0 + i) mod n), i < count; pi_key is a bijection of [0, n) for every n >= 1
 *   (a cycle-walked 6-round Feistel network whose round keys are a splitmix64 sequence started at `key`).
 * vqcpc_corpus_gather: window ids[r] = win_cum[p] + j (found by binary search) starts at beat o = j - (W - 1) of piece p; its tick
 *   t < W * subdivision is tick rel = o * subdivision + t of the piece: rel < -1 PAD, rel == -1 START, 0 <= rel < length the
 *   corpus row, rel == length END, rel > length PAD.  The 4 voices of tick t < split go, as int64, to out[r * ld_row + t * ld_tick
 *   + 0..3], those of t >= split to out2[r * ld_row2 + (t - split) * ld_tick2 + 0..3] (strides in int64 words; split =
 *   W * subdivision: out only, out2 may be null).  An id outside [0, win_cum[P]) writes nothing and stores 1 to *flag (int32).
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_corpus_permute(int64_t* ids, int64_t lo, int64_t n, uint64_t key, int64_t q0, int64_t count, void* stream);
int vqcpc_corpus_gather(const int32_t* tokens, const int64_t* piece_start, const int64_t* win_cum, const int32_t* special, int P,
                        int W, int subdivision, const int64_t* ids, int64_t count, int64_t* out, int64_t ld_row, int64_t ld_tick,
                        int split, int64_t* out2, int64_t ld_row2, int64_t ld_tick2, int32_t* flag, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Duplicate check: the longest common run of a token sequence against the corpus (csrc/duplicates.hip,
 * DeviceCorpus.longest_common_run; in place of the difflib loop of VQCPCB/decoders/decoder.py:983-1017).
 * DEFINITION.  Tokens are compared voice by voice in the flattened order (tick-major, voice-minor): query position
 *   i = 4 tick + voice is matched with corpus position j = 4 tick' + voice of the SAME voice, so j - i is a multiple of 4.  A run
 *   is a maximal stretch of consecutive equal tokens; it may begin and end in the middle of a tick and never crosses a piece
 *   boundary.  Only stored corpus ticks take part: the virtual PAD / START / END ticks of the window rule never match.  The
 *   answer per query row is the longest run; among equals the smallest i; among those the smallest j.  This is what
 *   difflib.SequenceMatcher(None, a, b, autojunk=False).find_longest_match gives per piece on lists of (voice, token) pairs,
 *   combined by (longest, smallest a, earliest piece).  The reference counts CHARACTERS of the dumped note names (so a long name
 *   counts more, a run may end inside a name, and its "(size - 1) / 3" assumes three characters per token) and compares with the
 *   padded windows, so padding in a generation counts as copied there; neither is reproduced.
 * FRAMED CORPUS.  One 64-bit word per tick, voice v in bits 16 v .. 16 v + 15, with one sentinel tick (all ones) in front of
 *   every piece and after the last: piece p starts at framed tick piece_start[p] + p + 1, n_framed = total_ticks + P + 1.  Tokens
 *   of queries and corpus are < 0xFFFF (the caller checks), so a sentinel equals nothing and runs break at piece boundaries.
 *   Any sub-array that starts and ends on a sentinel is the framed corpus of a contiguous piece range.
 * vqcpc_dup_frame: tokens (total_ticks, 4) int32, 16-byte aligned, and piece_start (P + 1) int64 -> framed (n_framed words).
 * vqcpc_dup_pack: int64 tokens x[g * ld_row + t * ld_tick + v] -> query[g * ld_query + t] in the word layout above.
 * vqcpc_dup_longest_run: out[g] = max(out[g], key) over the n_ticks + n_framed - 1 diagonals of row g, key =
 *   length << 48 | (0xFFFF - i) << 32 | (0xFFFFFFFF - j), j the token position inside `framed` (4 framed tick + voice); out
 *   (G uint64) is zeroed by the caller and 0 means no common token.  The maximum is order-independent: the result is
 *   deterministic.  Limits: n_ticks >= 1, 4 n_ticks <= 65535, 1 <= G <= 65535, 1 <= n_framed < 2^30, ld_query >= n_ticks.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_dup_frame(const int32_t* tokens, const int64_t* piece_start, int P, int64_t total_ticks, uint64_t* framed, void* stream);
int vqcpc_dup_pack(const int64_t* x, int64_t ld_row, int64_t ld_tick, int n_ticks, int G, uint64_t* query, int64_t ld_query,
                   void* stream);
int vqcpc_dup_longest_run(const uint64_t* framed, int64_t n_framed, const uint64_t* query, int64_t ld_query, int n_ticks, int G,
                          uint64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Cluster census: which rows every codeword collects, E examples per codeword, and the codewords next to each other
 * (csrc/clusters.hip, vqcpc_bach_amd/clusters.py; in place of the host loops of VQCPCB/encoder.py:112-185: `.item()` per block,
 * dict-of-lists grouping, random.shuffle and a cap of 50 in plot_clusters, norm + topk in show_nn_clusters).
 * DEFINITION.  A POPULATION is a set of rows, each with an id < 2^32 - 1 and one code per codebook, codes[row * ld + c] (int64,
 *   c < ncb <= 64, ld >= ncb), a code being in [0, K), K <= 2^24 (the merged code of a product quantiser is ncb = 1,
 *   K = codebook_size ** num_codebooks).  The COUNT of (c, k) is the number of rows whose code c is k.  The EXAMPLES of (c, k) are
 *   its E members with the smallest PACKED KEY h(key, id) << 32 | id, ascending, where
 *       h(key, id) = the low 32 bits of mix(key + id * 0x9E3779B97F4A7C15 mod 2^64),
 *       mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31   (mod 2^64; the
 *   splitmix64 finaliser of dataloaders/corpus.py mix_key; clusters.select_hash is the host twin).  Packed keys are unique -- the
 *   id sits in the low bits -- and none is all ones, the EMPTY slot value, because id < 2^32 - 1.  Counts and examples are functions
 *   of the SET of rows: the order of the rows, their split into calls and the scheduling of the threads do not enter.  The
 *   NEIGHBOURS of codeword i of a codebook are the k other codewords j != i of that codebook with the smallest
 *   (dist2(i, j), j), ascending; i is left out by index (the reference drops the first hit of topk(k + 1), which is another codeword
 *   when two coincide), and dist2 is the canonical chain of vqcpc_vq_fwd: acc = 0; for t ascending: df = e[i][t] - e[j][t],
 *   acc = acc + df * df, every operation rounded to fp32 on its own (no FMA), so a numpy float32 restatement gives the same bits.
 * vqcpc_cluster_count: counts[c * K + k] += count of (c, k) over the n rows; counts (ncb * K int32) is zeroed by the caller, so
 *   calls over disjoint row sets accumulate.  A code outside [0, K) is not counted and stores 1 to *flag (int32), as
 *   vqcpc_corpus_gather does.  ncb * K <= 8192: per-workgroup counts in LDS, one flush; larger: global integer atomics.
 *   Limits: 1 <= ncb <= 64, 1 <= K <= 2^24, ld >= ncb, 0 <= n < 2^31.
 * vqcpc_cluster_select: slots (ncb * K * E uint64, slot e of (c, k) at (c * K + k) * E + e) are set to all ones by the caller.
 *   After any number of calls over disjoint row sets slots[c][k][0 .. min(E, count) - 1] are the smallest packed keys of the
 *   members of (c, k), ascending, and the rest are still all ones.  The id of row r is ids[r] (int64) or, ids == null, id0 + r.  A
 *   row with a code outside [0, K) or an id outside [0, 2^32 - 1) takes no part and stores 1 to *flag.
 *   Limits: as vqcpc_cluster_count, 1 <= E <= 64, and without ids 0 <= id0, id0 + n <= 2^32 - 1.
 * vqcpc_codebook_knn: e (ncb, K, d) fp32, dense -> nn (ncb, K, k) int32 and dist2 (ncb, K, k) fp32, the neighbours above; finite
 *   codewords whose distances do not overflow.  Codebooks of more than 8192 floats are streamed through LDS in tiles.
 *   Limits: 1 <= ncb <= 65535, 2 <= K <= 2^24, 1 <= d <= 1024, 1 <= k <= 16, k < K.
 * No allocation or synchronisation in the launch functions; integer atomics and minima only: the results are deterministic.
 * Adding them left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_cluster_count(const int64_t* codes, int64_t ld, int64_t n, int ncb, int64_t K, int32_t* counts, int32_t* flag,
                        void* stream);
int vqcpc_cluster_select(const int64_t* codes, int64_t ld, int64_t n, int ncb, int64_t K, const int64_t* ids, int64_t id0,
                         uint64_t key, int E, uint64_t* slots, int32_t* flag, void* stream);
int vqcpc_codebook_knn(const float* e, int ncb, int K, int d, int k, int32_t* nn, float* dist2, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Particle resampling for constrained generation (csrc/particles.hip, decoders/generation.py; the rule is restated in numpy in
 * tests/particles_reference.py).  The M <= 64 rows of an incremental stack are G = M / P groups of P consecutive rows, 2 <= P <= 64.
 * vqcpc_particle_resample: ONE launch for all groups, after the U steps of a code.  c = w0 + pos[0] / U - 1 is the code's
 *   chorale index (w0 = win ? win[1] : 0, both read from device memory as the samplers read them); c < 0 (no live window,
 *   pos[0] < U): ancestors = the identity, flag = 0, nothing else is written.  Otherwise, per row b, in ascending q over the
 *   code's columns [c * U, (c + 1) * U):  lw[b] = lw[b] + logp[b * ldlogp + q] where constraint[b * ldcons + q] >= 0, else
 *   + logmass[b * ldmass + q] where logmass != NULL (one fp32 add each; NULL buffers and columns past a leading dimension add
 *   nothing).  NaN counts as -inf.  Per group, members ascending, every operation rounded on its own (no FMA contraction):
 *     mx = max lw, w = exp(lw - mx), s = sum w, wn = w / s, ess = 1 / sum wn^2, inc = (mx + log s) - log P;
 *   every member -inf: wn = 1 / P, inc = -inf, evidence[g] = -inf and the group is never resampled.
 *   A group resamples when force != 0 or ess < threshold * P:  u = (splitmix64(seeds[first row] ^ (c + 1) *
 *   0x8CB92BA72F3D8DD7) >> 40) * 2^-24; the ancestor of slot k is the first member j whose running fp32 sum of wn (ascending,
 *   sequential adds) exceeds (u + k) / P, else the last member; evidence[g] += inc and the group's lw become 0.  Otherwise
 *   the ancestors are the identity and lw keeps the sums.  Outputs: lw, evidence (G), pending (G) = inc, ancestors (M, int32,
 *   row indices of the stack), wn (M), ess (G), flag[0] = 1 if any ancestor differs from its own row else 0, and row c of the
 *   histories hist_ancestors (hist_rows, M), hist_wn (hist_rows, M), hist_ess (hist_rows, G) where given and c < hist_rows.
 * vqcpc_particle_permute_{i64,f32,cache}: row k <- row ancestors[k] of a buffer of M rows, IN PLACE, for every group; returns at
 *   once when flag[0] == 0.  A workgroup owns a column tile across all rows of a group, loads it into LDS and stores after
 *   the barrier, so cycles and fan-outs of the map are safe; an ancestor outside the row's group leaves the row alone.
 *   _i64 / _f32: buf [M][ld], columns [0, width) move, or [0, clamp(pos[0], 0, width)) when pos != NULL.  _cache: cache
 *   [layers][M][W][d] fp32 (a K or V cache of the stack), positions [0, clamp(pos[0], 0, W)) of every layer move; d % 4 == 0,
 *   16-byte aligned.  Rows at and beyond the bound, other groups and everything outside the buffer keep their bits.
 * No allocation or synchronisation in the launch functions.  Adding them left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_particle_resample(float* lw, float* evidence, float* pending, const int64_t* seeds, const int64_t* constraint,
                            int64_t ldcons, const float* logp, int64_t ldlogp, const float* logmass, int64_t ldmass,
                            const int32_t* pos, const int32_t* win, int U, float threshold, int force, int32_t* ancestors,
                            float* wn, float* ess, int32_t* flag, int32_t* hist_ancestors, float* hist_wn, float* hist_ess,
                            int64_t hist_rows, int64_t M, int P, void* stream);
int vqcpc_particle_permute_i64(int64_t* buf, int64_t ld, int64_t width, const int32_t* pos, const int32_t* ancestors,
                               const int32_t* flag, int64_t M, int P, void* stream);
int vqcpc_particle_permute_f32(float* buf, int64_t ld, int64_t width, const int32_t* pos, const int32_t* ancestors,
                               const int32_t* flag, int64_t M, int P, void* stream);
int vqcpc_particle_permute_cache(float* cache, int layers, int64_t W, int d, const int32_t* pos, const int32_t* ancestors,
                                 const int32_t* flag, int64_t M, int P, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Voice-leading rules as context-dependent token sets (csrc/rules.hip, decoders/generation.py `rules=`; the rule is restated in
 * numpy in tests/rules_reference.py).  Exact integer logic.  rules: a mask of CROSSING 1 | LEAP 2 | PARALLEL 4.  kinds [nc][ldk]
 * int32: per (voice, token) a MIDI pitch >= 0, HOLD -1, or REST / META below; max_leap [nc] int32 (< 0: off for that voice).
 * Voice 0 is the top voice.  Position: column col, tick e = col / nc, voice v = col % nc.
 * vqcpc_decode_rules: ONE launch, a wavefront per row, M <= 64, issued before vqcpc_decode_sample_masked inside the step.
 *   col = pos[0] (win == NULL) or win[1] * U + pos[0]; pos[0] outside [0, T) or win[1] < 0: nothing happens.  History = every
 *   column < col: tokens[b][c - win[1] * U] for c >= win[1] * U, else chorale[b][c].  pitch_at(u, e') walks back from tick e'
 *   while voice u holds (no bound but column 0).  prev_u = pitch_at(u, e - 1); the known voices are u < v (emitted) and u > v
 *   with constraint[b][e * nc + u] >= 0; now_u = the token's pitch, prev_u if it holds.  Candidate k of voice v with pitch p
 *   (prev_v if it holds) breaks CROSSING when p lies above a known upper or below a known lower voice, LEAP when it is a
 *   pitch further than max_leap[v] from prev_v, PARALLEL when v and a known u both move in the same direction from an
 *   interval of 0 or 7 (mod 12) to the same interval.
 *   Free position: E = static set (all of [0, V_v) without one) minus exclude[v]; while E has no candidate that breaks no
 *   remaining rule, PARALLEL, then LEAP, then CROSSING is dropped.  sets[b][col][0..8) = static & survivors, bits >= V_v zero
 *   (never empty inside the vocabulary: then the whole vocabulary is written); report[b][col] = the dropped enabled rules.
 *   Forced position: sets = the static set unchanged (the whole vocabulary without one); report = the enabled rules the forced
 *   token breaks, << 4.  Every write is a pure overwrite; a column at or past a leading dimension is not read / written.
 * vqcpc_rules_audit: x [rows][ld], width columns (a multiple of nc): every token is taken as forced and all history comes
 *   from x; report[b][c] = the enabled rules token c breaks, << 4 (0 where x < 0).  Grid of (column range, row).
 * The launch functions refuse, before any HIP call: NULL required pointers, M outside [1, 64], nc > 16, V_c > 256 or > ldk,
 * leading dimensions smaller than the widths.  No allocation or synchronisation.  Adding them left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_decode_rules(const int64_t* tokens, int64_t ldtok, int T, const int64_t* chorale, int64_t ldch, const int64_t* constraint,
                       int64_t ldcons, const int32_t* kinds, int ldk, const int32_t* voice_offsets, int nc, const int32_t* max_leap,
                       int rules, const uint32_t* exclude, const uint32_t* static_sets, int64_t ldstatic, uint32_t* sets,
                       int64_t ldsets, int32_t* report, int64_t ldreport, const int32_t* pos, const int32_t* win, int U, int64_t M,
                       void* stream);
int vqcpc_rules_audit(const int64_t* x, int64_t ld, int64_t width, const int32_t* kinds, int ldk, const int32_t* voice_offsets, int nc,
                      const int32_t* max_leap, int rules, int32_t* report, int64_t ldreport, int64_t rows, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Copy guard: token sets that keep a generation from reciting the corpus (csrc/nocopy.hip, decoders/generation.py `no_copy=`,
 * DeviceCorpus.copy_index; the rule is restated in numpy, without hashing, in tests/nocopy_reference.py).  Exact integer logic.
 * DEFINITION.  Everything follows the duplicate check above: positions are flattened tick-major, voice-minor; a query position is
 *   matched only with a corpus position of the same voice; a run never crosses a piece boundary; only stored corpus ticks take part
 *   (the virtual PAD / START / END never match); there are 4 voices.  With max_copy = n, token k is BANNED at column c (voice
 *   v = c % 4) of a row when c >= n and some corpus token position j satisfies all of: j has voice v; j - n .. j - 1 lie in j's own
 *   piece; corpus[j - m] == history[c - m] for m = 1 .. n; corpus[j] == k.  history is every column before c, read as
 *   vqcpc_decode_rules reads it: tokens[b][c' - win[1] * U] for c' >= win[1] * U, else chorale[b][c']; forced and free tokens are
 *   treated alike; a column that holds no token (< 0, >= 0xFFFF, at or past a leading dimension) equals nothing.  Emitting a banned
 *   token would complete a shared run of n + 1 tokens, so a row none of whose positions is flagged RELAXED or FORCED_COPY (below) has
 *   longest_common_run <= n.
 * THE INDEX.  `framed`: n_framed words of the duplicate check's framed corpus (a sub-array that starts and ends on a sentinel), read
 *   as 4 n_framed 16-bit tokens; token position j = 4 framed tick + voice.  An ENTRY is a position j >= n whose token is < 256 and
 *   whose n tokens before it hold no sentinel.  key = hash(voice, context) << 8 | token, a non-negative int64; `keys` sorted
 *   ascending, `where` the entries' positions in the same order.  The hash is not part of the contract: equal (voice, context) give
 *   equal hashes, and every candidate of a key range is compared token by token, so a collision costs a comparison and never a result.
 * vqcpc_copy_index_keys: keys[j] for every token position j < 4 n_framed: the entry's key, or -1 where j is no entry.
 * vqcpc_copy_index_unique: over SORTED keys / where (entries >= 1): keep[i] (bytes) = 0 where entry i - 1 has the same key and a
 *   context that compares equal, else 1.  Dropping the zeros leaves every (voice, context, token) at least once, and a context's
 *   range no longer than its distinct continuations plus whatever collisions interleave.
 * vqcpc_decode_nocopy: ONE launch, a wavefront per row, M <= 64, inside the step immediately before the sampler or
 *   vqcpc_decode_beam_select and after vqcpc_decode_rules.  col = pos[0] (win == NULL) or win[1] * U + pos[0]; pos[0] outside
 *   [0, T) or win[1] < 0: nothing happens.  in_set = copy_static[b][col] (NULL: the whole vocabulary [0, V_v); copy_static may be
 *   `sets` itself, in place, when the rule kernel wrote the column this step); an in_set without a token of the vocabulary is read
 *   as the whole vocabulary, as the samplers read it.  ban = the banned tokens (none when col < n).
 *   Free position: sets[b][col] = in_set & ~ban and copy_report[b][col] = |in_set & ban| (bits 0-8); if the ban removed something and
 *   left no token of [0, V_v) outside exclude[v], sets = in_set and copy_report = RELAXED (bit 16): the sampler never meets an
 *   empty set.  Forced position (constraint[b][col] >= 0): sets = in_set, copy_report = FORCED_COPY (bit 17) when the forced token is
 *   banned, else 0.  Every write is a pure overwrite; a column at or past a leading dimension is neither read nor written.
 * vqcpc_nocopy_audit: x [rows][ld], width columns (a multiple of 4): every token is taken as given and the history comes from x;
 *   report[b][c] = FORCED_COPY where token c completes a shared run of n + 1 tokens, else 0.  Grid of (column range, row).
 * vqcpc_nocopy_beam_column: after vqcpc_decode_beam_select (`flag`, `bound` = {pos, col} as it left them): where flag[0] != 0,
 *   copy_report[k][bound[1]] <- copy_report[ancestors[k]][bound[1]] for every row, in place, loads before stores.
 * The launch functions refuse, before any HIP call: NULL required pointers, M outside [1, 64], nc != 4, V_c > 256, max_copy outside
 * [1, 512], n_framed outside [1, 2^30), leading dimensions smaller than the widths.  No allocation or synchronisation.  Adding them
 * left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_copy_index_keys(const uint64_t* framed, int64_t n_framed, int max_copy, int64_t* keys, void* stream);
int vqcpc_copy_index_unique(const uint64_t* framed, int64_t n_framed, int max_copy, const int64_t* keys, const int64_t* where,
                            int64_t entries, uint8_t* keep, void* stream);
int vqcpc_decode_nocopy(const int64_t* tokens, int64_t ldtok, int T, const int64_t* chorale, int64_t ldch, const int64_t* constraint,
                        int64_t ldcons, const int64_t* keys, const int64_t* where, int64_t entries, const uint64_t* framed,
                        int64_t n_framed, int max_copy, const int32_t* voice_offsets, int nc, const uint32_t* exclude,
                        const uint32_t* copy_static, int64_t ldstatic, uint32_t* sets, int64_t ldsets, int32_t* copy_report,
                        int64_t ldreport, const int32_t* pos, const int32_t* win, int U, int64_t M, void* stream);
int vqcpc_nocopy_audit(const int64_t* x, int64_t ld, int64_t width, const int64_t* keys, const int64_t* where, int64_t entries,
                       const uint64_t* framed, int64_t n_framed, int max_copy, int32_t* report, int64_t ldreport, int64_t rows,
                       void* stream);
int vqcpc_nocopy_beam_column(int32_t* copy_report, int64_t ldreport, const int32_t* ancestors, const int32_t* flag, const int32_t* bound,
                             int64_t M, int W, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Beam search for decoder generation (csrc/beam.hip, decoders/generation.py `beam=W`; the rule is restated in numpy in
 * tests/beam_reference.py).  The M <= 64 rows of an incremental stack are G = M / W groups of W consecutive rows ("slots"), the
 * hypotheses of one user row, 1 <= W <= 64.
 * vqcpc_decode_beam_select: ONE launch for all groups, in the sampler's place at the end of a step.  p = pos[0], voice c = p % nc
 *   with V_c logits columns, column col = p (win == NULL) or win[1] * U + p, -1 when win[1] < 0 -- the samplers' rule.
 *   p outside [0, T): flag[0] = 0 and nothing else happens.
 *   Row log-probability: lp(b, v) = (logits[b][v] - m_b) - logf(s_b), m_b / s_b the row maximum and exp-sum over the voice's V_c
 *   columns, formed exactly as vqcpc_decode_sample_constrained forms logp (lane l holds tokens 4l .. 4l + 3, the same wave
 *   reductions): lp(b, v) has the bits that sampler writes for row b emitting v.
 *   Candidates of row b: at a forced column (constraint[b][col] >= 0) the one token, clamped to [0, V_c), exclusion and set
 *   ignored; at a free one the tokens of [0, V_c) in allowed[b][col] (no buffer, or no bit inside the vocabulary: all of them) that
 *   are not in exclude[c].  cand(b, v) = score[b] + lp(b, v), one fp32 add; NaN counts as -inf; live means cand > -inf.
 *   Per group the live candidates are ordered by cand descending, then row ascending, then token ascending.  Slot k < n (n = the
 *   number of live candidates, at most W) gets the k-th: ancestors[k] = its row, its token, score[k] = cand.  Slots k >= n are dead:
 *   slot 0's ancestor and token, score -inf.  n == 0: ancestors = the identity, every row emits its own lowest candidate token
 *   (token 0 without one), score -inf.  The caller starts a group with score 0 for its first row and -inf for the others.
 *   Written, all in slot order: tokens[k][p]; next_in row k = table row min(token * U + p % U, table_rows - 1); logp[k][col] =
 *   lp(ancestor, token); logmass[k][col] = the ancestor's (m_a - m) + logf(s_a) - logf(s) over its set, as the masked sampler forms
 *   it; rule_report[k][col] = the ancestor's value (every row is read before any is written); score (M); ancestors (M, int32 row
 *   indices of the stack); flag[0] = 1 if any ancestor differs from its own row else 0; row col of hist_ancestors (hist_rows, M)
 *   where given and col < hist_rows; bound[0] = p, bound[1] = col; then pos[0] = p + 1.  NULL buffers, col < 0 and a column at or
 *   past a leading dimension are free / not written.  cand_out (optional, [M][256]): every row's cand as the selection used it,
 *   -inf for a non-candidate.
 *   The moves row k <- row ancestors[k] that follow are vqcpc_particle_permute_* with P = W (none for W = 1): the tokens' columns
 *   [0, bound[0]), the record rows' columns [0, bound[1]) -- the live column is in slot order already -- and cache rows [0, pos[0]),
 *   position p's K/V having been written for the ancestor.
 *   Limits: 1 <= M <= 64, W dividing M, nc <= 16, V_c <= 256, d <= 4096.  One workgroup, no allocation or synchronisation.
 * Adding it left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_decode_beam_select(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t M, int W,
                             const uint32_t* exclude, const int64_t* constraint, int64_t ldcons, const uint32_t* allowed,
                             int64_t ldallow, float* logp, int64_t ldlogp, float* logmass, int64_t ldmass, int32_t* rule_report,
                             int64_t ldreport, const int32_t* win, int64_t* tokens, int64_t ldtok, int T, const float* table,
                             int64_t table_rows, int d, int U, float* next_in, int64_t ldn, float* score, int32_t* ancestors,
                             int32_t* flag, int32_t* bound, int32_t* hist_ancestors, int64_t hist_rows, float* cand_out,
                             int32_t* pos, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Beam search over the prior's code plans (csrc/prior_beam.hip, priors/generation.py `beam=W`; the rule is restated in numpy in
 * tests/prior_beam_reference.py).  Rows, groups and slots as for vqcpc_decode_beam_select, whose rule this is on a vocabulary of up
 * to 4096 merged codes.  Two launches take the sampler's place at the end of a step:
 * vqcpc_prior_beam_expand: one workgroup per row (256 threads, thread t owns codes 16t .. 16t + 15, vqcpc_prior_sample's layout).
 *   p = pos[0], column col = p (win == NULL) or win[1] + p, -1 when win[1] < 0 -- the constrained sampler's rule.  p outside
 *   [0, N): nothing is written.
 *   Row log-probability: lp(b, v) = (logits[b][v] - m_b) - logf(s_b), m_b / s_b the row maximum and exp-sum over the V columns,
 *   formed exactly as vqcpc_prior_sample_constrained forms logp (the raw row, thread-ascending sums, the same block reductions):
 *   lp(b, v) has the bits that sampler writes for row b emitting v.  row_mass[b] = (m_a - m) + logf(s_a) - logf(s) over the row's
 *   set allowed[b][col] ([M][ldallow][ceil(V / 32)] words), as vqcpc_prior_sample_masked forms logmass (0 without a set).
 *   Candidates of row b: at a forced column (constraint[b][col] >= 0) the one code, clamped to [0, V), the set ignored; at a free
 *   one the codes of [0, V) in the set (no buffer, or no bit inside the vocabulary: all of them).  cand(b, v) = score[b] + lp(b, v),
 *   one fp32 add; NaN counts as -inf; live means cand > -inf.
 *   Written: scratch_cand / scratch_code / scratch_lp (M, W): the row's min(W, live) best candidates in the order cand
 *   descending, then code ascending, the rest -inf / 0 / 0; row_mass (M); row_low (M) the row's lowest candidate code (0 without
 *   one) and row_lowlp (M) its lp.  cand_out (optional, [M][4096]): every row's cand as the selection used it, -inf for a
 *   non-candidate.
 * vqcpc_prior_beam_select: ONE workgroup for all groups, reading what the expansion wrote.  p and col as above; p outside [0, N):
 *   flag[0] = 0 and nothing else happens.  Per group the live candidates are ordered by cand descending, then row ascending, then
 *   code ascending.  Slot k < n (n = the number of live candidates, at most W) gets the k-th: ancestors[k] = its row, its code,
 *   score[k] = cand.  Slots k >= n are dead: slot 0's ancestor and code, score -inf.  n == 0: ancestors = the identity, every row
 *   emits its own lowest candidate code, score -inf.  The caller starts a group with score 0 for its first row and -inf for the
 *   others.
 *   Written, all in slot order: codes[k][p]; next_in row k = table row of the code; logp[k][col] = lp(ancestor, code);
 *   logmass[k][col] = row_mass[ancestor]; score (M); ancestors (M, int32 row indices of the stack); flag[0] = 1 if any ancestor
 *   differs from its own row else 0; row col of hist_ancestors (hist_rows, M) where given and col < hist_rows; bound[0] = p,
 *   bound[1] = col; then pos[0] = p + 1.  NULL buffers, col < 0 and a column at or past a leading dimension are free / not written.
 *   The moves row k <- row ancestors[k] that follow are vqcpc_particle_permute_* with P = W (none for W = 1): the codes' columns
 *   [0, bound[0]), the whole sequence, the record rows' columns [0, bound[1]) -- the live column is in slot order already -- and
 *   cache rows [0, pos[0]), position p's K/V having been written for the ancestor.
 * Limits are vqcpc_prior_sample's: V <= 4096, 1 <= M <= 64, N <= 1024, d <= 4096; 1 <= W <= 64 dividing M.  The launch functions
 * refuse NULL required pointers and leading dimensions smaller than the widths before any HIP call.  No allocation or
 * synchronisation.
 * vqcpc_prior_beam_expand_product / vqcpc_prior_beam_select_product: the same two kernel bodies for ONE DIGIT STAGE of a product
 *   prior (1 <= ncb <= 4 codebooks of K <= 4096, K^ncb + 1 < 2^31; code = sum_j digit_j K^j), launched as a pair per stage j = 0 ..
 *   ncb - 1 of a position: the search prunes to the group's W best (row, digit) pairs AFTER EVERY DIGIT -- a beam over the digit
 *   sequence, not over the K^ncb merged codes.  With ncb = 1 every output equals the merged pair's bit for bit.
 *   expand, stage j: logits are the stage's K logits, lp / row_mass as above with V = K; `base` is what the stage adds to: the
 *   hypotheses' scores at stage 0, the previous stage's stage_score afterwards (cand = base[b] + lp).  From stage 1 on the rows
 *   are in slot order, so the constraint and the digit sets of row b are those of the stack row it descends from, anc_in[b] (the
 *   previous select's anc_total; ignored at stage 0).  A forced code (clamped to the K^ncb codes) gives its digit j as the one
 *   candidate; otherwise the candidates are the digits of allowed[row][col][j] ([M][ldallow][ncb][ceil(K / 32)] words), all K where
 *   the set has no digit inside.
 *   select, a stage before the last: the slot rule above on (row, digit) pairs; written per slot k, every value of an ancestor
 *   read before any is written: digits[k][0..j] (M, ncb) = the ancestor's digits with digit j appended; logp_acc[k] and mass_acc[k]
 *   -- stage 0 stores lp / the ancestor's row_mass, later stages add theirs with one fp32 add in ascending stage order, the chain
 *   of vqcpc_prior_sample_product(_masked) --; stage_score[k] = cand (-inf for a dead slot); anc_total[k] = the stack row the
 *   slot descends from, composed over the stages (stage 0: the ancestor itself); h_next[k] = h[ancestor] + dtab[j][digit] (h and
 *   h_next are different buffers).  codes, next_in, logp, logmass, score, ancestors, flag, bound, hist_ancestors and pos are
 *   left alone.
 *   select, the last stage: what vqcpc_prior_beam_select writes, with codes[k][p] = the merged code of the slot's digits, next_in
 *   the left-to-right sum of the digits' rows of tables [ncb][K][d] (the chain of vqcpc_product_gather), logp / logmass from the
 *   accumulators plus this stage's, and ancestors / hist_ancestors / flag from the composition over all stages; then pos + 1.
 *   p outside [0, N): the last stage sets flag[0] = 0, nothing else happens.
 * Adding them left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_prior_beam_expand(const float* logits, int64_t ldl, int V, int64_t M, int W, const int64_t* constraint, int64_t ldcons,
                            const uint32_t* allowed, int64_t ldallow, const int32_t* win, const float* score, int N,
                            const int32_t* pos, float* scratch_cand, int32_t* scratch_code, float* scratch_lp, float* row_mass,
                            int32_t* row_low, float* row_lowlp, float* cand_out, void* stream);
int vqcpc_prior_beam_select(const float* scratch_cand, const int32_t* scratch_code, const float* scratch_lp, const float* row_mass,
                            const int32_t* row_low, const float* row_lowlp, int V, int64_t M, int W, float* logp, int64_t ldlogp,
                            float* logmass, int64_t ldmass, const int32_t* win, int64_t* codes, int64_t ldc, int N,
                            const float* table, int64_t table_rows, int d, float* next_in, int64_t ldn, float* score,
                            int32_t* ancestors, int32_t* flag, int32_t* bound, int32_t* hist_ancestors, int64_t hist_rows,
                            int32_t* pos, void* stream);
int vqcpc_prior_beam_expand_product(const float* logits, int64_t ldl, int K, int ncb, int stage, int64_t M, int W,
                                    const int64_t* constraint, int64_t ldcons, const uint32_t* allowed, int64_t ldallow,
                                    const int32_t* win, const float* base, const int32_t* anc_in, int N, const int32_t* pos,
                                    float* scratch_cand, int32_t* scratch_code, float* scratch_lp, float* row_mass,
                                    int32_t* row_low, float* row_lowlp, float* cand_out, void* stream);
int vqcpc_prior_beam_select_product(const float* scratch_cand, const int32_t* scratch_code, const float* scratch_lp,
                                    const float* row_mass, const int32_t* row_low, const float* row_lowlp, int K, int ncb, int stage,
                                    int64_t M, int W, int32_t* digits, float* logp_acc, float* mass_acc, float* stage_score,
                                    int32_t* anc_total, const float* h, int64_t ldh, const float* dtab, float* h_next, int64_t ldhn,
                                    float* logp, int64_t ldlogp, float* logmass, int64_t ldmass, const int32_t* win, int64_t* codes,
                                    int64_t ldc, int N, const float* tables, int d, float* next_in, int64_t ldn, float* score,
                                    int32_t* ancestors, int32_t* flag, int32_t* bound, int32_t* hist_ancestors, int64_t hist_rows,
                                    int32_t* pos, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Scoring given tokens under the decoder (csrc/score.hip, decoders/scoring.py `Decoder.score_tokens`; the outputs are restated in
 * numpy float64 in tests/score_reference.py).
 * vqcpc_decode_score: ONE launch scores R independent rows of logits (R, ldl) in the samplers' layout (all voices concatenated,
 *   voice_offsets [nc + 1]); a wavefront per row, four rows per workgroup, no LDS.  Row r belongs to piece b = row_b[r] and chorale
 *   column col = row_col[r] (device int32 [R]); its voice is c = col % nc with V_c logits columns, only those are read.  A row with
 *   col outside [0, cols) or b outside [0, B) is skipped: nothing is read or written for it.  Target t = chorale[b][col] (int64,
 *   [B][ldch]), clamped to [0, V_c) as the samplers clamp a forced token.  Every output is optional (NULL: not computed) and is
 *   written at [b * ld + col] of its own [B][ld] array, nowhere else:
 *     logp      float32  (x_t - m) - logf(s), m / s the row maximum and exp-sum over the V_c columns, formed exactly as
 *               vqcpc_decode_sample_constrained forms logp (lane l holds tokens 4l .. 4l + 3, a lane-serial sum of four, the same
 *               wave reductions): the bits that sampler writes for this row with t forced
 *     logmass   float32  (m_a - m) + logf(s_a) - logf(s) over the set allowed[b][col][0..8) (uint32 words, [B][ldallow][8], bit
 *               i & 31 of word i >> 5), formed exactly as vqcpc_decode_sample_masked forms it: its bits.  Only bits [0, V_c) count,
 *               a set without any is no restriction, allowed == NULL is the full set; the full set gives exactly 0
 *     entropy   float32  -sum_i p_i log p_i in nats over the V_c tokens, as logf(s) + (sum_i e_i (m - x_i)) / s with e_i = expf(x_i - m):
 *               every term is >= 0; the sums in the order above
 *     rank      int32    #{i < V_c : x_i > x_t or (x_i == x_t and i < t)}: 0 = the model's first choice.  Exact
 *     best      int64    the arg-max over [0, V_c), the lowest index among equals.  Exact
 *     best_logp float32  logp formed for `best`
 *   A row's results depend on nothing but its own logits, set and target: a row alone gives the bits it gives among others.
 *   The launch function refuses, before any HIP call: NULL required pointers, nc > 16, V_c outside [1, 256], R, B or cols < 1,
 *   ldl smaller than the voices' widths, ldch, ld or (with allowed) ldallow smaller than cols.  No allocation or synchronisation.
 * Adding it left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_decode_score(const float* logits, int64_t ldl, const int32_t* voice_offsets, int nc, int64_t R, const int32_t* row_b,
                       const int32_t* row_col, const int64_t* chorale, int64_t ldch, const uint32_t* allowed, int64_t ldallow,
                       int64_t B, int64_t cols, int64_t ld, float* logp, float* logmass, float* entropy, int32_t* rank, int64_t* best,
                       float* best_logp, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Scoring given codes under the prior (csrc/prior_score.hip, priors/scoring.py `PriorRelative.score_codes(method='windows')`; the
 * outputs are restated in numpy float64 in tests/prior_score_reference.py).
 * vqcpc_prior_score: ONE launch scores R >= 1 independent rows of logits (R, ldl) with 1 <= V <= 4096 columns; R is not bounded by the
 *   samplers' 64.  Row r belongs to piece b = row_b[r] and sequence column col = row_col[r] (device int32 [R]).  A row with col
 *   outside [0, cols) or b outside [0, B) is skipped: nothing is read or written for it.  The target t is the code seq[b][col]
 *   (int64, [B][ldseq]) clamped to [0, V^ncb) as vqcpc_prior_sample_constrained clamps a forced code; with ncb > 1 the row is
 *   stage `stage` of a product code (V = K) and t is digit `stage` of the clamped code, (code / K^stage) % K, the digit rule of
 *   vqcpc_prior_sample_product.  Every output is optional (NULL: not computed):
 *     logp      float32  [b * ldlogp + col]             (x_t - m) - logf(s), m / s the row maximum and exp-sum over the V columns,
 *               formed exactly as vqcpc_prior_sample_constrained forms logp (thread t owns codes 16t .. 16t + 15 and sums them in
 *               ascending order, then the wave butterfly and (w0 + w1) + (w2 + w3); a -inf logit contributes 0, a -inf target
 *               gives -inf): the bits that sampler writes for this row with t forced.  Stage 0 stores; stage j >= 1 writes
 *               old + own (one fp32 add), so that ncb launches in ascending stage order on one stream leave the bits of
 *               vqcpc_prior_sample_product's logp_acc chain
 *     entropy   float32  [b * ld + col * ncb + stage]   -sum_i p_i log p_i in nats over the V codes, as logf(s) + (sum_i e_i (m - x_i)) / s
 *               with e_i = expf(x_i - m); every term is >= 0, a -inf logit contributes 0; the sums in the order above
 *     rank      int32    [b * ld + col * ncb + stage]   #{i < V : x_i > x_t or (x_i == x_t and i < t)}: 0 = the model's first choice.  Exact
 *     best      int64    [b * ld + col * ncb + stage]   the arg-max over [0, V), the lowest index among equals.  Exact
 *     best_logp float32  [b * ld + col * ncb + stage]   logp's formula at `best`
 *   A row's results depend on nothing but its own logits and target: a row alone gives the bits it gives among others.  Rows of
 *   V <= 1024 codes are scored by a wavefront each (the other three wavefronts of the sampler's tree hold zeros and -inf there:
 *   the same bits), larger rows by a workgroup of 256 threads each; the row is read once.
 *   The launch function refuses, before any HIP call: NULL logits, row_b, row_col or seq, V outside [1, 4096], ncb outside [1, 4],
 *   stage outside [0, ncb), V^ncb >= 2^31, R, B or cols < 1, ldl < V, ldseq < cols, (with logp) ldlogp < cols, (with any other
 *   output) ld < cols * ncb.  No allocation, no synchronisation, no atomics.
 * Adding it left the ABI version alone.
 * ------------------------------------------------------------------------------------------------------------------ */
int vqcpc_prior_score(const float* logits, int64_t ldl, int V, int ncb, int stage, int64_t R, const int32_t* row_b,
                      const int32_t* row_col, const int64_t* seq, int64_t ldseq, int64_t B, int64_t cols, float* logp,
                      int64_t ldlogp, int64_t ld, float* entropy, int32_t* rank, int64_t* best, float* best_logp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQCPC_H */
