/* uds_hip.h -- C ABI of libuds_hip.so, the MI355X (gfx950) message-passing engine for the
 * GNN-UDS graph-convolution hot path.
 *
 * The reference (Zhiyu014/GNN-UDS) has no FFI: its seam is the Keras layer protocol
 * (SURVEY.md section 8b).  Each entry point below replaces the TensorFlow ops behind one
 * reference call site (file:line relative to the reference's surrogate/ directory):
 *
 *   uds_dense_act            keras Dense                        emulator.py:198,203,206,212,225-226,278-279,313,317,324,329-330,336
 *                            + the "...NI,IHO->...NHO" node-update einsum of Spektral GATConv (via emulator.py:229-230)
 *   uds_csr_spmm             NodeEdge.call on its support       emulator.py:42-45 (used at :227-228,280-281)
 *                            + GCNConv propagation a_hat @ (xW) emulator.py:131-134
 *                            + post_proc_tf incidence matmuls   emulator.py:717-724
 *   uds_gat_forward          MixedGAT(GATConv)([x, adj])        emulator.py:18-25,229-230,282-283
 *   uds_spatial_layer_forward  one spatial-block loop body      emulator.py:225-230 / 278-283
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer owned by the caller (fp32, row-major, contiguous,
 *     16-byte aligned); `rowptr`/`col` passed to uds_csr_create are HOST pointers and are copied;
 *   - snapshots: S = B*T independent graph signals share one graph; node features are (S, N, F);
 *   - all launches are asynchronous on `stream` (a hipStream_t; 0 = the null stream); the library
 *     never synchronises, never allocates after handle creation (graph-capture safe) and starts
 *     no host threads; handles are immutable after creation and may be shared across streams;
 *   - return value 0 = success, negative errno-style code otherwise; nothing throws across the
 *     boundary; uds_last_error() gives the thread-local message of the last failure.
 */
#ifndef UDS_HIP_H
#define UDS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UDS_ABI_VERSION 23

enum {
  UDS_OK = 0,
  UDS_EINVAL = -22, /* bad argument (shape, alignment, null pointer)   */
  UDS_ENOMEM = -12, /* device allocation failed                         */
  UDS_EHIP = -5,    /* a HIP runtime call failed (see uds_last_error)   */
  UDS_ENOSYS = -38  /* configuration not built into this library        */
};

/* keras.activations names used by the reference (emulator.py:66,193,324,330,336) */
enum {
  UDS_ACT_LINEAR = 0,
  UDS_ACT_RELU = 1,
  UDS_ACT_TANH = 2,
  UDS_ACT_SIGMOID = 3,
  UDS_ACT_HARD_SIGMOID = 4 /* Keras 2.10: clip(0.2*x + 0.5, 0, 1) */
};

typedef void *uds_stream_t; /* hipStream_t */

int uds_abi_version(void);
const char *uds_last_error(void);

/* ---- CSR pattern handle ------------------------------------------------------------------- */
typedef struct uds_csr uds_csr_t;

/* Copies a host CSR pattern (int32, rowptr[n_rows+1], col[nnz] < n_cols) to the device and builds
 * the degree-sorted row schedule (descending degree, ties by row index). */
int uds_csr_create(const int32_t *rowptr, const int32_t *col, int64_t n_rows, int64_t n_cols,
                   int64_t nnz, uds_csr_t **out);
int uds_csr_destroy(uds_csr_t *csr);
int uds_csr_shape(const uds_csr_t *csr, int64_t *n_rows, int64_t *n_cols, int64_t *nnz,
                  int32_t *max_degree);
/* Copies the row schedule (n_rows int32) to a HOST buffer: integer bookkeeping, tested bit-exact. */
int uds_csr_row_order(const uds_csr_t *csr, int32_t *out_host);

/* ---- single ops ---------------------------------------------------------------------------- */

/* out[r,:] = act([xa[r,:] | xb[r,:]] @ W + bias), r < rows.   W is (fa+fb, f_out) row-major.
 * xb may be NULL with fb = 0; bias may be NULL.  When a_self/a_nbr (f_out each) are given,
 * s_self[r] = <pre-activation row, a_self> and s_nbr[r] likewise are written too (the GAT
 * attention scalars); they must be NULL together.
 * Alignment: `out` must be 16-byte aligned when f_out % 4 == 0 (float4 stores), else UDS_EINVAL.  No other operand has to
 * be.  The narrow-input kernel (below) loads W and bias as float4, so it runs only when both are 16-byte aligned; a
 * misaligned W or bias runs on the tiled kernel, which reads them with scalar loads and gives the same bits. */
int uds_dense_act(const float *xa, int64_t fa, const float *xb, int64_t fb, int64_t rows,
                  const float *W, const float *bias, int64_t f_out, int act, const float *a_self,
                  const float *a_nbr, float *out, float *s_self, float *s_nbr,
                  uds_stream_t stream);

/* Which kernel uds_dense_act (taps = 0) or uds_conv1d_causal (taps > 0: fa = F, fb = 0, f_out = H, rows = B * T * R) runs
 * for a shape, and over which grid.  Host only (works without a GPU); the launch decides with the same code.
 *   attn        non-zero when the attention scalars are asked for
 *   wb_aligned  non-zero when W and bias (NULL counts as aligned) are 16-byte aligned
 *   info5 = {kernel, parameter, rows per workgroup, workgroups launched, grid stride in lanes}
 *     kernel 0  the tiled kernel k_dense_act<CG>: parameter = CG, the power of two >= ceil(f_out / 4) in 1 .. 64; a workgroup
 *               owns 128 rows (CG <= 8), 64 (16), 32 (32) or 16 (64); the stride is 0
 *     kernel 1  the narrow-input stream k_embed_act<F>: parameter = F = fa.  Taken when fb = 0, taps = 0, no attention
 *               scalars, fa <= 8, f_out % 4 == 0, rows >= 64 and wb_aligned.  One lane per float4 of the output, at most
 *               4096 workgroups of 256 lanes, their number a multiple of (f_out / 4) / gcd(256, f_out / 4) so that the
 *               stride, 256 * workgroups, is a multiple of f_out / 4; rows per workgroup is 0
 * UDS_EINVAL for the sizes the two entries refuse, and for a grid of more than 2^31 - 1 workgroups. */
int uds_dense_route(int64_t fa, int64_t fb, int64_t taps, int attn, int64_t f_out, int64_t rows, int wb_aligned,
                    int32_t *info5);

/* out[s,r,:] = act(sum_{p in row r} val[p] * x[s, col[p], :] + bias);  x is (S, n_cols, F),
 * out is (S, n_rows, F).  val (nnz) may be NULL (all ones); bias (F) may be NULL.  F % 4 == 0. */
int uds_csr_spmm(const uds_csr_t *csr, const float *val, const float *x, int64_t S, int64_t F,
                 const float *bias, int act, float *out, uds_stream_t stream);

/* keras Conv1D(H, taps, padding='causal', dilation_rate=dil, activation) along T on x laid out (B, T, R, F) with no
 * transposes: out[b,t,r,:] = act(sum_j x[b, t-(taps-1-j)*dil, r, :] @ kernel[j] + bias), zero outside [0, T).
 * dil < 0 looks ahead instead of back: with kernel[j] transposed this is the input gradient of the causal layer.
 * kernel is (taps, F, H) row-major (the Keras layout); out is (B, T, R, H).   emulator.py:155-157,244-257,299-310 */
int uds_conv1d_causal(const float *x, int64_t B, int64_t T, int64_t R, int64_t F, const float *kernel,
                      const float *bias, int64_t taps, int64_t dil, int64_t H, int act, float *out,
                      uds_stream_t stream);

/* The time recurrence of keras GRU / LSTM(H, return_sequences=True) (emulator.py:158-161, the `recurrent` alternatives to
 * the causal Conv1D), exact fp32.  xp (B, T, R, G*H) = x @ kernel + input bias for every time step (uds_dense_act), U
 * (H, G*H) the recurrent kernel, rb (G*H) the recurrent bias or NULL; kind 0 = GRU (G = 3, gate order z, r, h, TF2's
 * reset_after=True form, sigmoid recurrent activation), 1 = LSTM (G = 4: i, f, c, o).  out (B, T, R, H) = the hidden state
 * after every step, initial state zero.  H <= 256.  Where H * G*H floats fit the LDS (a GRU up to 116 units, an LSTM up to
 * 100) U is staged there once per workgroup; above that it is streamed from global memory, the same arithmetic. */
int uds_recurrent_forward(const float *xp, const float *U, const float *rb, int64_t B, int64_t T, int64_t R, int64_t H,
                          int kind, float *out, uds_stream_t stream);

/* The same recurrence for a training step (emulator.py:457-484: fit_eval differentiates through the GRU / LSTM layers of
 * get_tem_nets, emulator.py:158-161; `recurrent: GRU` is the default of every block of utils/config.yaml): c_out (B, T, R, H)
 * additionally receives the LSTM's cell state after every step (NULL: not kept; ignored for the GRU).
 *
 * uds_recurrent_backward: back-propagation through time of a 64-unit layer, one launch on the matrix cores (split-bf16);
 * uds_recurrent_backward_h below is the same for every width from 16 to 128.
 * xp, h (the forward output), c (the LSTM's cell states, NULL for the GRU) and gh = dL/dh, all (B, T, R, .) as above;
 * packed = the G 64-column slices of U in uds_rowgemm_pack layout followed by the G slices of U_g^T (16 KiB each).
 * Outputs: dxp (B, T, R, G*64) = gradient of the input projection (the Dense backward takes it from there: dW = x^T dxp,
 * d b_in = sum dxp, dx = dxp W^T) and darec (G, B, T, R, 64) = gradient of the recurrent pre-activation h[t-1] U + b_rec,
 * gate-major so that dU[:, 64g:64g+64] = sum_t h[t-1]^T darec[g][t] is one uds_wgrad call with a time shift of 1 and
 * d b_rec its bias row. */
int uds_recurrent_forward_train(const float *xp, const float *U, const float *rb, int64_t B, int64_t T, int64_t R, int64_t H,
                                int kind, float *out, float *c_out, uds_stream_t stream);
int uds_recurrent_backward(const float *xp, const void *packed, const float *b_rec, const float *h, const float *c,
                           const float *gh, int64_t B, int64_t T, int64_t R, int kind, float *dxp, float *darec,
                           uds_stream_t stream);

/* uds_recurrent_backward for a layer of H units, H a multiple of 16 from 16 to 128 (`hidden_dim` of utils/config.yaml is the
 * width of every temporal layer: emulator.py:158-161 under the GradientTape of fit_eval, emulator.py:457-484).  Arguments
 * and outputs as uds_recurrent_backward with 64 replaced by H: xp / dxp (B, T, R, G*H), h / c / gh (B, T, R, H), b_rec (G*H)
 * or NULL, darec (G, B, T, R, H).  H = 64 is uds_recurrent_backward itself (the same kernel, launch and bits).
 * packed = uds_recurrent_pack_bwd(U (H, G*H) row-major), uds_recurrent_bwd_packed_bytes(H, kind) bytes (0: width or kind not
 * supported): the G slices U[:, gH:(g+1)H], then the G slices of their transposes, each ceil(H / 32) k-steps x H / 16
 * feature blocks of bf16 hi / lo MFMA fragments, [(kt * H/16 + m) * 2 + hl] * 64 + lane, 16 bytes each, the K rows from H up
 * to 32 ceil(H / 32) zero.  At H = 64 that is the image uds_recurrent_backward takes.  Up to 64 units the image is staged in
 * LDS once per workgroup; above (180 KiB and more) the kernel reads each fragment from it in place, so it must stay valid
 * until the launch has finished. */
int64_t uds_recurrent_bwd_packed_bytes(int64_t H, int kind);
int uds_recurrent_pack_bwd(const float *U, int64_t H, int kind, void *packed, uds_stream_t stream);
int uds_recurrent_backward_h(const float *xp, const void *packed, const float *b_rec, const float *h, const float *c,
                             const float *gh, int64_t B, int64_t T, int64_t R, int64_t H, int kind, float *dxp,
                             float *darec, uds_stream_t stream);

/* A whole keras GRU / LSTM(64, return_sequences=True) layer in ONE launch on the matrix cores (split-bf16, three products,
 * fp32 accumulation): input projection, recurrent product, gates and state update per time step, the state fed back from
 * the accumulator registers; out (B, T, R, 64) = the hidden state after every step.   emulator.py:158-161 (`recurrent: GRU`
 * is the reference's default).
 *   F = 64 or 128: x (B, T, R, F) are the input rows; `packed` = uds_rowgemm_pack of the G 64-column slices of `kernel`
 *                  (F, G*64), then of `recurrent_kernel` (64, G*64), back to back; b_in (G*64) the input bias.
 *   F = 0:         x (B, T, R, G*64) is the input projection `x @ kernel + bias` itself (any input width, computed by
 *                  uds_rowgemm_forward_cat); `packed` holds the recurrent slices only; b_in is not read (for the GRU fold the
 *                  recurrent bias of the z and r gates into the projection's bias).
 * b_rec (G*64): the recurrent bias of the TF2 GRU (reset_after=True), NULL for the LSTM; kind 0 = GRU (G = 3: z, r, h),
 * 1 = LSTM (G = 4: i, f, c, o).  uds_recurrent_fused_supported(F, kind): whether W + U of that form fit the LDS. */
int uds_recurrent_fused_supported(int64_t F, int kind);
int uds_recurrent_fused(const float *x, int64_t F, const void *packed, const float *b_in, const float *b_rec, int64_t B,
                        int64_t T, int64_t R, int kind, float *out, uds_stream_t stream);

/* Matrix-core version of uds_dense_act (taps = 1, T = 1: rows = B*R) and uds_conv1d_causal for F % 32 == 0 and
 * f_out <= 64: operands split into bf16 hi + lo, three MFMA products, fp32 accumulation (the fused spatial kernel's
 * numerics).  `packed` = uds_rowgemm_pack(W (taps*F, f_out)) -- uds_rowgemm_packed_bytes() bytes, once per
 * parameter update.                                              emulator.py:155-157,313,317,324,329-330,336 */
int64_t uds_rowgemm_packed_bytes(int64_t k_total, int64_t f_out);
int uds_rowgemm_pack(const float *W, int64_t k_total, int64_t f_out, void *packed, uds_stream_t stream);
int uds_rowgemm_forward(const float *x, int64_t B, int64_t T, int64_t R, int64_t F, const void *packed,
                        const float *bias, int64_t taps, int64_t dil, int64_t f_out, int act, float *out,
                        uds_stream_t stream);

/* Two uds_rowgemm_forward problems of the same layer shape (B, T, F, taps, dil, f_out, act) in ONE launch when both are
 * small (<= 16 384 rows each: an autoregressive step on a 2k-node network), else as two launches: the node-side and the
 * link-side temporal layer of a step (emulator.py:244-257) -- problem i: x_i (B, T, R_i, F) -> out_i (B, T, R_i, f_out). */
int uds_rowgemm_forward_pair(const float *x0, int64_t R0, const void *packed0, const float *bias0, float *out0,
                             const float *x1, int64_t R1, const void *packed1, const float *bias1, float *out1, int64_t B,
                             int64_t T, int64_t F, int64_t taps, int64_t dil, int64_t f_out, int act, uds_stream_t stream);

/* uds_rowgemm_forward whose input row is the concatenation [x (F1) | x2 (F2)] of two tensors (x2 NULL, F2 = 0: one
 * tensor; two tensors need taps = 1) and whose f_out outputs go to columns [col0, col0 + f_out) of rows of `ldo`
 * floats: a 128-wide layer is two calls on the two column halves of its kernel, no concatenation copies
 * (`concat([x, NodeEdge(x_e)])` -> GATConv kernel, emulator.py:227-230 at embed_size = 128). */
int uds_rowgemm_forward_cat(const float *x, int64_t F1, const float *x2, int64_t F2, int64_t B, int64_t T, int64_t R,
                            const void *packed, const float *bias, int64_t taps, int64_t dil, int64_t f_out, int act,
                            float *out, int64_t ldo, int64_t col0, uds_stream_t stream);

/* spektral DiffusionConv as the reference runs it (dense mixed mode, emulator.py:135-138,229): channel q is
 * reduce_sum(polyval(theta_q, a_hat) @ x, -1) with tf.math.polyval applied to the ENTRIES of a_hat, so zero entries take the
 * constant coefficient c0[q] and the N x N product collapses to the CSR support:
 *   out[s, i, q] = act( c0[q] * tot[s] + sum_{p in row i} vals[p, q] * r[s, col[p]] ),
 * r[s, j] = sum_f x[s, j, f] (S, n_cols), tot[s] = sum_j r[s, j] (S), vals[p, q] = polyval(theta_q, a_p) - c0[q] (nnz, C),
 * out (S, n_rows, C), C % 4 == 0. */
int uds_diffusion_forward(const uds_csr_t *csr, const float *vals, const float *c0, const float *r, const float *tot,
                          int64_t S, int64_t C, int act, float *out, uds_stream_t stream);

/* The reverse of uds_diffusion_forward (training a DiffusionConv), exact fp32, in three launches; no atomics, so two calls on
 * the same inputs give the same bits.  With gz = act'(y) * gy (act' from the forward's output y, as autograd.act_grad),
 * K1 = K + 1 coefficients per channel (highest power first), M_0[s, i] = tot[s], M_m[s, i] = sum_{p in row i} a[p]^m r[s, col[p]]:
 *   dtheta[q, k] = sum_{s, i} gz[s, i, q] * M_{K-k}[s, i]                                   (C, K1), overwritten
 *   dr[s, j]     = sum_{i, q} c0[q] gz[s, i, q] + sum_{p : col[p] = j} sum_q vals[p, q] gz[s, row(p), q]    (S, n_cols)
 * dr is the gradient of r (tot = sum_j r[s, j] is folded in: its term reaches every j); dx[s, j, f] = dr[s, j] for every f.
 * csr: the pattern of the forward; csr_t: its transpose (n_cols rows); perm_t (int32, nnz): perm_t[p] = position in csr's
 * row-major order of entry p of csr_t (CsrHandle.transposed), entries < nnz (not checked on the device).  a (nnz): the values
 * a_hat takes on the support, in csr's order.  vals (nnz, C), c0 (C), r (S, n_cols), tot (S) as uds_diffusion_forward;
 * y, gy (S, n_rows, C).  C % 4 == 0, C <= 256, 1 <= K1 <= 16, S <= 65535; vals, c0, y, gy and workspace 16-byte aligned.
 * workspace: uds_diffusion_backward_workspace_floats(n_rows, S, C, K1) floats (gz and per-block partials; -1 for sizes the
 * kernels do not take). */
int64_t uds_diffusion_backward_workspace_floats(int64_t n_rows, int64_t S, int64_t C, int64_t K1);
int uds_diffusion_backward(const uds_csr_t *csr, const uds_csr_t *csr_t, const int32_t *perm_t, const float *a, const float *vals,
                           const float *c0, const float *r, const float *tot, const float *y, const float *gy, int64_t S, int64_t C,
                           int64_t K1, int act, float *workspace, float *dr, float *dtheta, uds_stream_t stream);

/* uds_diffusion_forward / uds_diffusion_backward without the (nnz, C) table `vals` (spektral DiffusionConv, emulator.py:135-138,229):
 * the polynomial is expanded per ROW instead of per entry.  theta (C, K1): the layer's kernel, row q = theta_q, highest power
 * first (K = K1 - 1, c0[q] = theta[q][K]); a (nnz): the values a_hat takes on the support.  With the row moments
 *   M_0[s, i] = tot[s],   M_m[s, i] = sum_{p in row i} a[p]^m r[s, col[p]]   (m = 1..K; powers by running product, p ascending)
 *   out[s, i, q] = act( sum_{m = 0..K} theta[q][K - m] * M_m[s, i] )          (m ascending)
 * and in reverse, with gz = act'(y) * gy and G_m[s, i] = sum_q theta[q][K - m] gz[s, i, q]:
 *   dtheta[q, k] = sum_{s, i} gz[s, i, q] * M_{K-k}[s, i]          -- the launches of uds_diffusion_backward: the same bits
 *   dr[s, j]     = sum_i G_0[s, i] + sum_{p : col[p] = j} sum_{m = 1..K} a[p]^m G_m[s, row(p)]
 * Reads a, r and theta (held in LDS) where the table entries read nnz * C floats per snapshot.  Same contract as the table
 * entries: C % 4 == 0, C <= 256, 1 <= K1 <= 16, S <= 65535; theta, out, y, gy and workspace 16-byte aligned; exact fp32, no
 * atomics (two calls give the same bits), no allocation or synchronisation.  csr_t / perm_t as uds_diffusion_backward;
 * workspace: uds_diffusion_backward_m_workspace_floats(n_rows, S, C, K1) floats (-1 for sizes the kernels do not take). */
int uds_diffusion_forward_m(const uds_csr_t *csr, const float *a, const float *theta, const float *r, const float *tot,
                            int64_t S, int64_t C, int64_t K1, int act, float *out, uds_stream_t stream);
int64_t uds_diffusion_backward_m_workspace_floats(int64_t n_rows, int64_t S, int64_t C, int64_t K1);
int uds_diffusion_backward_m(const uds_csr_t *csr, const uds_csr_t *csr_t, const int32_t *perm_t, const float *a,
                             const float *theta, const float *r, const float *tot, const float *y, const float *gy,
                             int64_t S, int64_t C, int64_t K1, int act, float *workspace, float *dr, float *dtheta,
                             uds_stream_t stream);

/* Message buffers of the graph-sharded spatial block (one 200k-node network node-cut over the GPUs; the reference holds
 * whole graphs on one device, SURVEY.md F5 / 8e -- the exchange itself is torch.distributed isend / irecv over RCCL).
 *   pack:   buf[s, i, :] = i < nx ? x[s, idx_x[i], :] : e[s, idx_e[i - nx], :]     one buffer per peer, node rows then link rows
 *   unpack: the inverse scatter into rows idx_x of x and idx_e of e (the halo rows the peer owns).
 * x (S, n_x, F), e (S, n_e, F), buf (S, nx + ne, F), F % 4 == 0; idx_* are int32 device arrays of LOCAL row numbers. */
int uds_halo_pack(const float *x, int64_t n_x, const float *e, int64_t n_e, int64_t S, int64_t F, const int32_t *idx_x,
                  int64_t nx, const int32_t *idx_e, int64_t ne, float *buf, uds_stream_t stream);
int uds_halo_unpack(const float *buf, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx, const int32_t *idx_e,
                    int64_t ne, float *x, int64_t n_x, float *e, int64_t n_e, uds_stream_t stream);

/* The messages of ALL P peers of one exchange in one launch each way (the whole-Emulator graph-sharded forward).
 * idx_x (nx) / idx_e (ne) are the peers' row lists concatenated; peer q's rows are idx_x[off_x[q] .. off_x[q+1]) and
 * idx_e[off_e[q] .. off_e[q+1]) (off_* int32 device arrays of P + 1 non-decreasing offsets, off_*[0] = 0, off_x[P] = nx,
 * off_e[P] = ne; a peer may have no rows).  One buffer: peer q's message is the contiguous (S, nx_q + ne_q, F) block at
 * float offset S * F * (off_x[q] + off_e[q]), node rows then link rows, as uds_halo_pack lays out one message.
 *   pack_all:   every block filled from x (S, n_x, F) / e (S, n_e, F)
 *   unpack_all: the inverse scatter (in place)
 * Any F >= 1 (16-byte vector path when F % 4 == 0 and x, e, buf are 16-byte aligned, per-float otherwise); S <= 65535;
 * idx_* are LOCAL row numbers < n_x / n_e (not checked on the device).  UDS_EINVAL on bad sizes or NULL arguments,
 * UDS_EHIP when the launch fails. */
int uds_halo_pack_all(const float *x, int64_t n_x, const float *e, int64_t n_e, int64_t S, int64_t F, const int32_t *idx_x,
                      int64_t nx, const int32_t *idx_e, int64_t ne, const int32_t *off_x, const int32_t *off_e, int64_t P,
                      float *buf, uds_stream_t stream);
int uds_halo_unpack_all(const float *buf, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx, const int32_t *idx_e,
                        int64_t ne, const int32_t *off_x, const int32_t *off_e, int64_t P, float *x, int64_t n_x, float *e,
                        int64_t n_e, uds_stream_t stream);

/* The adjoint of uds_halo_unpack_all (gradients across the node cut, graph-sharded training), in two launches.
 *   pack_clear_all:  as uds_halo_pack_all (same arguments, same buffer layout), and every source element is set to 0
 *                    after it is read -- a halo row whose value the exchange overwrote returns its gradient to the owner
 *                    and keeps none.  The rows listed across all peers must be distinct (not checked on the device).
 *   accumulate_all:  the owner ADDS what its peers returned.  buf is laid out by off_x / off_e (P + 1 offsets) as
 *                    uds_halo_pack_all lays it out; message rows are numbered across peers, peer q's rows
 *                    off_x[q] + off_e[q] + j, node rows first.  Targets: tx rows tgt_x of x then te rows tgt_e of e,
 *                    distinct; target t (node targets numbered first) adds the message rows src[ptr[t] .. ptr[t+1])
 *                    (ptr: tx + te + 1 offsets, n_src = ptr[tx + te]) in the listed order, ascending peer:
 *                      row[s, :] = ((row[s, :] + m_0[s, :]) + m_1[s, :]) + ...
 *                    No atomics: the result is bitwise reproducible and independent of message arrival order.
 * x (S, n_x, F), e (S, n_e, F); any F >= 1 (16-byte vector path when F % 4 == 0 and x, e, buf are 16-byte aligned,
 * per-float otherwise); S <= 65535; all int32 arrays are on the device and their rows are not checked there.
 * UDS_EINVAL on bad sizes or NULL arguments, UDS_EHIP when the launch fails. */
int uds_halo_pack_clear_all(float *x, int64_t n_x, float *e, int64_t n_e, int64_t S, int64_t F, const int32_t *idx_x, int64_t nx,
                            const int32_t *idx_e, int64_t ne, const int32_t *off_x, const int32_t *off_e, int64_t P, float *buf,
                            uds_stream_t stream);
int uds_halo_accumulate_all(const float *buf, int64_t S, int64_t F, const int32_t *off_x, const int32_t *off_e, int64_t P,
                            const int32_t *tgt_x, int64_t tx, const int32_t *tgt_e, int64_t te, const int32_t *ptr,
                            const int32_t *src, int64_t n_src, float *x, int64_t n_x, float *e, int64_t n_e,
                            uds_stream_t stream);

/* Dense remainder of a TRAINED NodeEdge layer.  The reference's layer is `(w * inci + b) @ x` with w, b dense trainable
 * (R, M) matrices (emulator.py:34-45); on the incidence support that is the CSR aggregation of the fused kernel, off the
 * support it is `rest @ x`, rest = b with the support entries zeroed -- a true (R x M) x (M x S*h) GEMM.  Matrix cores,
 * split-bf16 (three products, fp32 accumulation):
 *   out[s, r, :] = sum_m rest[r, m] * x[s, m, :]        x (S, M, h), out (S, R, h), h % 4 == 0, h <= 64.
 * `packed` = uds_remainder_pack(rest), uds_remainder_packed_bytes(R, M) bytes, once per parameter update; `workspace` =
 * uds_remainder_workspace_bytes(R, M, S, h) bytes of scratch per call (the transposed bf16 image of x, and the accumulator
 * pieces of the tiles k_remainder_gemm2 cuts along K: at most 128 MiB). */
int64_t uds_remainder_packed_bytes(int64_t R, int64_t M);
int uds_remainder_pack(const float *rest, int64_t R, int64_t M, void *packed, uds_stream_t stream);
int64_t uds_remainder_workspace_bytes(int64_t R, int64_t M, int64_t S, int64_t h);
int uds_remainder_forward(const void *packed, int64_t R, int64_t M, const float *x, int64_t S, int64_t h, void *workspace,
                          float *out, uds_stream_t stream);

/* The same with the activations computed on the way: out = rest @ act(e W + b) for e (S, M, F), F = 64 or 128, W (F x h, packed by
 * uds_rowgemm_pack), h = 32 or 64.  In a trained layer x_e = Dense(e) exists only to be multiplied by `rest` (emulator.py:225-228 with
 * :36-45): this entry writes it straight into the GEMM's bf16 operand planes instead of an fp32 tensor that is then read back, split
 * and transposed.  Same workspace as uds_remainder_forward. */
int uds_remainder_forward_dense(const void *packed, int64_t R, int64_t M, const float *e, int64_t F, const void *packed_w,
                                const float *bias, int act, int64_t S, int64_t h, void *workspace, float *out,
                                uds_stream_t stream);

/* The same product for the networks the reference ships (tens to a few hundred rows), in ONE launch and without a workspace: a
 * workgroup computes x_e = act(e W + b) of G consecutive snapshots into an LDS image, multiplies it by `rest` (streamed from the
 * planes of uds_remainder_pack, the same `packed` as above) and writes out (S, R, h) once.  F = 64 or 128, h = 32 or 64; no host
 * synchronisation and no allocation (capturable).
 * uds_remainder_snapshot_plan is host only (works without a GPU): info4 = {G = snapshots per workgroup, 0 when the shape is refused
 * (M above 576: the image of 64 columns does not fit the LDS; F or h out of range), LDS bytes, row blocks per wave pass, 0}.
 * The launch entries return UDS_EINVAL for what the plan refuses.  uds_remainder_snapshot_pair runs two problems that share F, h,
 * act and S -- the node side and the link side of one layer -- in one launch; a side whose `packed` is NULL is skipped (both NULL
 * is an error). */
int uds_remainder_snapshot_plan(int64_t R, int64_t M, int64_t F, int64_t h, int32_t *info4);
int uds_remainder_snapshot(const void *packed, int64_t R, int64_t M, const float *e, int64_t F, const void *packed_w,
                           const float *bias, int act, int64_t S, int64_t h, float *out, uds_stream_t stream);
int uds_remainder_snapshot_pair(const void *packed0, int64_t R0, int64_t M0, const float *e0, const void *packed_w0,
                                const float *bias0, float *out0, const void *packed1, int64_t R1, int64_t M1, const float *e1,
                                const void *packed_w1, const float *bias1, float *out1, int64_t F, int act, int64_t S, int64_t h,
                                uds_stream_t stream);

/* keras Dense(64) (64 inputs) + prefix sum over time + residual + activation in one pass (matrix cores, split-bf16):
 *   out[b,t,r,:] = act( sum_{t' <= t} (x[b,t',r,:] @ kernel + bias) + res[b,0,r,:] ),   x, out: (B,T,R,64), res: (B,1,R,64) or NULL.
 * `packed` = uds_rowgemm_pack of the (64, 64) kernel.  The `dense_resx` layer and the `cumsum(x_out, axis=1) + res` that
 * follows it (emulator.py:313-320): one read and one write of the tensor instead of two each. */
int uds_dense_cumsum(const float *x, int64_t B, int64_t T, int64_t R, const void *packed, const float *bias,
                     const float *res, int act, float *out, uds_stream_t stream);

/* uds_dense_cumsum with the emulator's output heads as its epilogue (emulator.py:313-338): the 64-wide resnet output
 *   y = act(cumsum_t(x @ kernel + bias) + res)
 * is consumed where it is produced and never written: out[b,t,r,:] = [ act_a(y @ A + a_bias)  (n_a <= 4 columns)  |
 * act_f(h_n @ F + f_bias)  (1 column, only when n_hidden > 0) ] with h_0 = y, h_i = act_h(h_{i-1} @ H_i + h_bias_i), H_1
 * (64, 32), H_2 .. H_5 (32, 32; n_hidden <= 5): the `out` head + the flood chain on the node side (:324-333), the `e_out` head alone on the
 * link side (:336).  Every *_packed is uds_rowgemm_pack of that layer's kernel.  out (B, T, R, n_a + (n_hidden > 0)). */
typedef struct {
  const void *a_packed;    /* (64, n_a) */
  const float *a_bias;     /* n_a floats or NULL */
  const void *h_packed[5]; /* (64, 32), then up to four (32, 32); unused entries NULL */
  const float *h_bias[5];  /* 32 floats each or NULL */
  const void *f_packed;    /* (32, 1) */
  const float *f_bias;     /* 1 float or NULL */
  int32_t n_a, act_a, n_hidden, act_h, act_f;
} uds_heads_t;
int uds_dense_cumsum_heads(const float *x, int64_t B, int64_t T, int64_t R, const void *packed, const float *bias,
                           const float *res, int act, const uds_heads_t *heads, float *out, uds_stream_t stream);

/* A whole temporal stack in one launch: n_layers (2 or 3) causal Conv1D(64 -> 64, kernel 3, dilation 2^i) layers with one
 * activation applied back to back to x (B,T,R,64) -> out (B,T,R,64); the layers in between never reach memory (`tem1_x`,
 * `tem1_e`, `tem2_x`, `tem2_e`).  packed[i] = uds_rowgemm_pack of layer i's (3*64, 64) kernel, bias[i] 64 floats or NULL.
 * Bit-identical to n_layers uds_rowgemm_forward calls (taps 3, dil 2^i) on the streaming-Conv1D route.  Time is cut into n_seg
 * segments, each of which re-computes a halo of sum_i 2 * 2^i steps (6 / 14): n_seg = 0 takes uds_conv_stack_plan's, else
 * 1 <= n_seg <= T is used as given (the result does not depend on it).  `out` must not overlap `x`.  Any number of rows: whether
 * the launch pays is the caller's call.  uds_conv_stack_plan is host only (no device).
 *                                                                            emulator.py:154-157,244-257,299-310 */
typedef struct {
  const void *packed[3];
  const float *bias[3];
  int32_t n_layers, act;
} uds_conv_stack_t;
int uds_conv_stack_plan(int64_t B, int64_t T, int64_t R, int n_layers, int64_t *n_seg, int64_t *seg_len, int64_t *halo);
int uds_conv_stack_forward(const float *x, int64_t B, int64_t T, int64_t R, const uds_conv_stack_t *layers, int64_t n_seg,
                           float *out, uds_stream_t stream);

/* out[b,t,r,:] = act(cumsum_t(x)[b,t,r,:] + res[b,0,r,:]); x, out (B,T,R,F), res (B,1,R,F) or NULL; F % 4 == 0.
 * The resnet head of the emulator.                                          emulator.py:313-320 */
int uds_cumsum_act(const float *x, const float *res, int64_t B, int64_t T, int64_t R, int64_t F, int act,
                   float *out, uds_stream_t stream);

/* spektral GlobalAttnSumPool in batch mode, the head of the RL agents' graph encoder (agent.py:93-94, `ConvNet`):
 * out[b, :] = sum_r softmax_r(<x[b, r, :], k>) x[b, r, :] for x (B, R, F), k (F), F a power of two up to 256.  One pass over the
 * rows (online softmax), fixed merge order: bitwise reproducible. */
int uds_attn_sum_pool(const float *x, const float *k, int64_t B, int64_t R, int64_t F, float *out, uds_stream_t stream);

/* The same pool over two row blocks, without the concatenation `ConvNet` used to build for it: per sample b the rows are those of
 * x[b] (Rx, F) followed by those of e[b] (Re, F); e may be NULL with Re = 0.  With s_r = <row_r, k>, M = max_r s_r, L = sum_r
 * exp(s_r - M), alpha_r = exp(s_r - M) / L: out[b, :] = sum_r alpha_r row_r, and stat (B, 2), when not NULL, receives (M, L) for
 * the backward.  Every row is visited at the step and with the operations of uds_attn_sum_pool on the stacked tensor: `out` is
 * bit for bit that entry's result.  F a power of two from 4 to 256, x / e / k / out 16-byte aligned. */
int uds_attn_sum_pool_pair(const float *x, int64_t Rx, const float *e, int64_t Re, const float *k, int64_t B, int64_t F, float *out,
                           float *stat, uds_stream_t stream);

/* Reverse mode of uds_attn_sum_pool_pair from its saved out (B, F) and stat (B, 2), for the upstream gradient grad (B, F).  With
 * g = grad[b] and t_r = <g, row_r> - <g, out[b]>:
 *   ds_r = alpha_r t_r,   d row_r = alpha_r g + ds_r k  (dx (B, Rx, F) / de (B, Re, F)),   dk (F) = sum_b sum_r ds_r row_r
 * alpha_r is recomputed from the row and (M, L): nothing of size (B, R) is stored.  One pass: x / e are read once, dx / de
 * written once.  dk is summed without float atomics -- per-sample partial sums go to the caller's workspace dk_ws (B, F), a
 * second launch adds them over b in a fixed order -- so a second call gives the same bits.  dx, de and dk may each be NULL
 * (that gradient is not computed; dk_ws is needed only with dk).  Limits and alignment as uds_attn_sum_pool_pair. */
int uds_attn_sum_pool_backward(const float *x, int64_t Rx, const float *e, int64_t Re, const float *k, const float *out,
                               const float *stat, const float *grad, int64_t B, int64_t F, float *dx, float *de, float *dk_ws,
                               float *dk, uds_stream_t stream);

/* keras Dropout in training mode (the emulator's Dropout(0.2) / Dropout(self.dropout) layers,   emulator.py:199-213,234-235,
 * 287-288,314-318; `self.model(inp, training=fit)`, :411,434): out[i] = x[i] / (1 - rate) if element i is kept, else 0, for n floats;
 * out may be x.  0 <= rate < 1.  The mask is a pure function of (seed, offset + i) -- Philox4x32-10, key = seed, counter =
 * (offset + i) / 4, word (offset + i) % 4, kept when word >= rate * 2^32 -- so the backward pass is the same call on the gradient
 * with the same (seed, offset) and nothing is stored; the caller advances offset by n per use. */
int uds_dropout(const float *x, int64_t n, float rate, uint64_t seed, uint64_t offset, float *out, uds_stream_t stream);

/* Link -> node flow balance of post_proc_tf: inc_n is the (N x E) incidence support, sign (nnz) its +1 / -1 values,
 * flow (S,E) the signed link flows; q_in, q_out (S,N) are scaled per node by scale_in / scale_out (N).
 * q_out = inc+ @ max(f,0) + inc- @ max(-f,0),  q_in = inc- @ max(f,0) + inc+ @ max(-f,0).   emulator.py:717-724 */
int uds_flow_balance(const uds_csr_t *inc_n, const float *sign, const float *flow, int64_t S,
                     const float *scale_in, const float *scale_out, float *q_in, float *q_out,
                     uds_stream_t stream);

/* One chunk of the autoregressive rollout after the forward (Emulator._model, emulator.py:403-423, with the edge-fusion
 * branch of post_proc_tf, :717-724): flow = ey[..., ce-1] * span_e + mini_e (de-normalised link flow, per link), q_in /
 * q_out as uds_flow_balance, preds (B,so,N,cy+2) = [y[...,0], q_in, q_out, y[...,1:]]; then both state windows are shifted
 * by `so` steps IN PLACE and fed with the prediction: x (B,T,N,cy+3) gets [preds with the last y channel, y[...,cy-1] > 0.5 ?
 * 1 : 0, in place of its value when flood != 0 and cy >= 2 (the flood bit is a y channel of its own after the depth: with
 * cy = 1 nothing is thresholded), b], ex (B,T,E,ce+1) gets [ey, 1].  y (B,so,N,cy), ey (B,so,E,ce), b (B,so,N,1); the kept
 * T - so steps of both windows are the old steps so .. T-1 (none when so = T).  Bit-identical to the tensor-by-tensor
 * composition. */
int uds_roll_update(const uds_csr_t *inc_n, const float *sign, const float *span_e, const float *mini_e,
                    const float *scale_in, const float *scale_out, const float *y, int64_t cy, const float *ey,
                    int64_t ce, const float *b, int64_t B, int64_t so, int64_t T, int flood, float *x, float *ex,
                    float *preds, uds_stream_t stream);

/* Constants of the predict tail (uds_predict_tail): everything Emulator._predict does after the network forward.  All
 * pointers are device memory, fp32 / int32, built once per model (gnn_uds_amd/emulator.py: Emulator._tail_params); a table
 * whose switch is off is not read but must still be given.  C = 3 + (if_flood != 0) is the channel count of the
 * de-normalised node row [h, q_in, q_out, (flood)]; cy, the channel count of the network output, is C - 2 with edge_fusion
 * (q_in / q_out come from the link flows) and C without. */
typedef struct uds_tail {
  /* sizes */
  int32_t N, E, cy, ce, n_act, b_channels;
  /* switches (0 / 1) */
  int32_t edge_fusion, tide, has_offset, act, pump_override, any_pump, if_flood;
  /* scalars: depth_gate = the depth above which a node pump runs (0 in predict_tf, 0.01 in predict); epsilon as the model's */
  float depth_gate, epsilon;
  /* per node (N): area_eps = area + 1e-6, ps = the pumped-storage mask, ny_in / ny_out = norm_y[0, :, 1 / 2],
   * scale_in / scale_out = (ny > 1e-3) / ny; span_y / mini_y (N, C) = max - min / min of norm_y */
  const float *is_outfall, *hmin, *hmax, *area_eps, *ps, *pump_in, *pump_out, *ny_in, *ny_out, *scale_in, *scale_out;
  const float *span_y, *mini_y;
  /* per link (E): pump_den = norm_e[0, :, 2], pump_mask = pump_den > 1e-3; from_node / from_ok = the link's from-node and
   * whether it has one (a link from a node to itself has none); span_e / mini_e (E, ce) */
  const float *offset, *pump, *pump_mask, *pump_den, *ehmax, *from_ok;
  const float *span_e, *mini_e;
  const int32_t *from_node;
  /* settings: act_link (E) / act_in / act_out (N) = 1 + the action that sets the link / gates the node's inflow / outflow,
   * 0 = none */
  const int32_t *act_link, *act_in, *act_out;
  /* backward only: the (up to) two incidence entries of every link, link_node (E, 2) (-1 = none) and link_sign (E, 2); and per
   * action the links / inflow nodes / outflow nodes it drives as CSR lists (ptr: n_act + 1) */
  const int32_t *link_node;
  const float *link_sign;
  const int32_t *al_ptr, *al_idx, *ai_ptr, *ai_idx, *ao_ptr, *ao_idx;
} uds_tail_t;

/* The tail of Emulator.predict_tf / predict (emulator.py:811-903) in two launches: tide, offset gate, rated-pump override,
 * edge and node action gates, link -> node flow balance (as uds_flow_balance), de-normalisation, ehmax clamp, pumped-storage
 * depth scan over T and constrain_tf.  y (B,T,N,cy) and ey (B,T,E,ce) are the network outputs, a (B,T,n_act) the settings
 * (NULL without act), b_norm (B,T,N,b_channels) the normalised boundary (its last channel is the tide), runoff (B,T,N) the raw
 * runoff, h0 (B,N) the last known depth.  out_y (B,T,N,C+1) = [h, q_in, q_out, (flood), q_w], out_ey (B,T,E,ce).  2 <= ce <= 8.
 * Same operations in the same order as the tensor code, no fused multiply-add: bit-identical to it. */
int uds_predict_tail(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey,
                     const float *a, const float *b_norm, const float *runoff, const float *h0, int64_t B, int64_t T,
                     float *out_y, float *out_ey, uds_stream_t stream);

/* Floats of workspace uds_predict_tail_backward needs. */
int64_t uds_predict_tail_workspace_floats(int64_t N, int64_t E, int64_t B, int64_t T);

/* Reverse mode of uds_predict_tail for the upstream gradients g_out_y / g_out_ey: dy, dey, da (NULL without act), dh0 in the
 * shapes of y, ey, a, h0.  Two launches plus one per-action reduction, no atomics: deterministic.  Comparisons carry no
 * gradient; max / min split evenly at a tie; clamp(min = 0) passes at 0; the flow balance passes nothing at a flow of 0. */
int uds_predict_tail_backward(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y,
                              const float *ey, const float *a, const float *b_norm, const float *runoff,
                              const float *h0, int64_t B, int64_t T, const float *g_out_y, const float *g_out_ey,
                              float *dy, float *dey, float *da, float *dh0, float *workspace, uds_stream_t stream);

/* The tail of a training step: everything Emulator.fit_eval / fit_grad_norm do after the network forward (emulator.py:400-484)
 * -- post_proc_tf (tide, offset gate, rated-pump override, link and node action gates, link -> node flow balance), clamp(0, 1),
 * get_node_loss (balance != 0: through constrain_tf, emulator.py:441-447), the weighted flood BCE (if_flood without balance) and
 * the link MSE -- in three launches.  p as for uds_predict_tail, with depth_gate = 0 and pump_override = "every link is a pump";
 * area_eps, ps, ehmax and the per-action lists are not read.  y, ey, a: as there; b_norm (B,T,N,b_channels) the normalised
 * boundary (channel 0 the runoff, the last one the tide); y_true (B,T,N,cyt) = [h, q_in, q_out, .., (flood at cyt - 2), q_w at
 * cyt - 1], cyt >= 3; ey_true (B,T,E,ce); nwei (N, 3 + balance), poswei (N), ewei (E) the loss weights; qw_den (N) =
 * norm_y[0, :, -1], span_b / mini_b (N) = max - min / min of the runoff norm (read with balance only).
 * out_y (B,T,N,C) and out_ey (B,T,E,ce) are what post_proc_tf returns (normalised, NOT clamped: the rollout feeds them back),
 * bit-identical to the tensor code.  loss_sums[3] = [node, flood, edge]: the sums of the per-sample terms of the three losses on
 * clamp(out_y, 0, 1) before the division by the sample count (flood: 0 unless if_flood without balance).  Probabilities are clipped
 * to [1e-7, 1 - 1e-7].  Per-workgroup partials in `workspace`, then a fixed-order second stage: no atomics, the same bits every
 * run. */
int uds_fit_tail(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey,
                 const float *a, const float *b_norm, const float *y_true, const float *ey_true, const float *nwei,
                 const float *poswei, const float *ewei, const float *qw_den, const float *span_b, const float *mini_b,
                 int64_t B, int64_t T, int64_t cyt, int balance, float *out_y, float *out_ey, float *loss_sums,
                 float *workspace, uds_stream_t stream);

/* Floats of workspace uds_fit_tail and uds_fit_tail_backward need (one size serves both). */
int64_t uds_fit_tail_workspace_floats(int64_t N, int64_t E, int64_t B, int64_t T);

/* Reverse mode of uds_fit_tail (emulator.py:400-484 under the tape): dy and dey in the shapes of y and ey for g_loss[3], the
 * gradients of the three loss sums (device memory: no host round trip), plus g_out_y / g_out_ey, the gradients arriving at the two
 * outputs through the rollout's feedback (either may be NULL: none).  The gates are recomputed from y and ey.  clamp(0, 1) and the
 * probability clip pass on their closed intervals, comparisons carry nothing, max / min split evenly at a tie, the flow balance
 * passes nothing at a flow of 0.  Not differentiable in a, b_norm or the targets.  Two launches, no atomics. */
int uds_fit_tail_backward(const uds_csr_t *inc_n, const float *sign, const uds_tail_t *p, const float *y, const float *ey,
                          const float *a, const float *b_norm, const float *y_true, const float *ey_true,
                          const float *nwei, const float *poswei, const float *ewei, const float *qw_den,
                          const float *span_b, const float *mini_b, int64_t B, int64_t T, int64_t cyt, int balance,
                          const float *g_loss, const float *g_out_y, const float *g_out_ey, float *dy, float *dey,
                          float *workspace, uds_stream_t stream);

/* Floats of workspace uds_gat_forward needs: S * n * (d + 2). */
int64_t uds_gat_workspace_floats(int64_t n, int64_t S, int64_t d);

/* Single-head GATConv on a CSR pattern that already contains the self loops:
 *   hx = [xa | xb] @ W              (W: (fa+fb, d))
 *   alpha_ij = softmax_j leaky_relu_0.2( <hx_i, a_self> + <hx_j, a_nbr> ),  j in row i
 *   out_i = act( sum_j alpha_ij hx_j + bias )
 * xa:(S,n,fa), xb:(S,n,fb) or NULL, out:(S,n,d), d % 4 == 0. */
int uds_gat_forward(const uds_csr_t *graph, const float *xa, int64_t fa, const float *xb,
                    int64_t fb, int64_t S, const float *W, const float *a_self,
                    const float *a_nbr, const float *bias, int64_t d, int act, float *workspace,
                    float *out, uds_stream_t stream);

/* The attention / aggregation half of uds_gat_forward on its own: hx (S,n,d) = the transformed features, s_self / s_nbr
 * (S,n) = their projections on the two attention kernels, however the caller computed them (e.g. with the matrix-core
 * row GEMM for wide layers: d = 128 is the reference's default embed_size).
 *   out_i = act( sum_j softmax_j(leaky_relu_0.2(s_self_i + s_nbr_j)) hx_j + bias ),  j in row i of `graph`. */
int uds_gat_aggregate(const uds_csr_t *graph, const float *hx, const float *s_self, const float *s_nbr,
                      const float *bias, int64_t S, int64_t d, int act, float *out, uds_stream_t stream);

/* ---- reverse mode of the sparse operators (the GradientTape of fit_eval, emulator.py:457-484) ---------- */

/* uds_gat_aggregate with a per-snapshot edge mask: the `use_adj` variant, where the control action rewrites the adjacency
 * entries of the actuated links at every time step and GAT casts the result to int (a setting < 1 removes the entry) --
 * emulator.py:268-271,343-362.  edge_mask (S, nnz) floats in the pattern's entry order: entry p of snapshot s takes part
 * iff edge_mask[s, p] != 0 or it is the diagonal (spektral sets the diagonal to one after the rewrite). */
int uds_gat_aggregate_masked(const uds_csr_t *graph, const float *hx, const float *s_self, const float *s_nbr,
                             const float *bias, const float *edge_mask, int64_t S, int64_t d, int act, float *out,
                             uds_stream_t stream);

/* Attention part of uds_gat_forward, backwards.  With pre_i = sum_j alpha_ij hx_j (before bias / activation) and
 * grad = dL/dpre (S,n,d), hx / s_self / s_nbr as uds_gat_forward left them in its workspace:
 *   d_hx (S,n,d)   = dL/dhx (aggregation + both attention scores),
 *   ds_self, ds_nbr (S,n) = dL/ds_self, dL/ds_nbr  (for the gradients of the attention kernels: sum hx * ds),
 * graph_t = the transposed pattern as its own handle, perm_t (device, nnz int32) = for every entry of graph_t the
 * position of the same entry in graph's row-major order.  alpha_ws / de_ws: S * nnz floats of workspace each.
 * Replaces the tape through spektral GATConv._call_dense (emulator.py:229-230,282-283). */
int uds_gat_backward(const uds_csr_t *graph, const uds_csr_t *graph_t, const int32_t *perm_t, const float *grad,
                     const float *hx, const float *s_self, const float *s_nbr, const float *a_self,
                     const float *a_nbr, int64_t S, int64_t d, float *alpha_ws, float *de_ws, float *d_hx,
                     float *ds_self, float *ds_nbr, uds_stream_t stream);

/* The two entries above with Spektral's ATTENTION DROPOUT (GATConv: `attn_coef_drop = dropout(softmax(...))`, rate 0.5, which the
 * reference switches on together with the model's Dropout layers: `self.model(inp, training=fit)`, emulator.py:411,434):
 * coef (S, nnz) multiplies the normalised coefficient of entry p of snapshot s (0 or 1 / (1 - rate); uds_dropout on a tensor of
 * ones makes it).  Forward: out_i = act(sum_j alpha_ij coef_ij hx_j + bias); backward: the same workspace and outputs as
 * uds_gat_backward.  Training path only. */
int uds_gat_aggregate_coef(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias,
                           const float *coef, int64_t S, int64_t d, int act, float *out, uds_stream_t stream);
int uds_gat_backward_coef(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad, const float *hx,
                          const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr, const float *coef,
                          int64_t S, int64_t d, float *alpha_ws, float *de_ws, float *d_hx, float *ds_self, float *ds_nbr,
                          uds_stream_t stream);

/* uds_gat_aggregate with an optional per-snapshot EDGE MASK and an optional attention-dropout COEF, for training `use_adj`
 * models (emulator.py:268-271,343-362: the action rewrites the adjacency entries of the actuated links per time step and GAT
 * casts them to int, so a setting < 1 removes the entry; the training step, emulator.py:457-484, differentiates through it).
 * edge_mask (S, nnz) or NULL: entry p of snapshot s takes part iff edge_mask[s, p] != 0 or p is its row's diagonal (spektral
 * restores the diagonal with set_diag after the rewrite).  The softmax runs over the surviving entries only (a masked logit
 * is -10e9 in the reference: its weight is exactly 0).  coef (S, nnz) or NULL multiplies the normalised coefficients as in
 * uds_gat_aggregate_coef.  With an all-ones mask and no coef the result is bitwise that of uds_gat_aggregate. */
int uds_gat_aggregate_ex(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias,
                         const float *edge_mask, const float *coef, int64_t S, int64_t d, int act, float *out,
                         uds_stream_t stream);
/* Reverse mode of uds_gat_aggregate_ex: arguments and outputs as uds_gat_backward_coef, plus the same edge_mask (or NULL).
 * A masked entry has alpha = de = 0 in the workspace, so it contributes nothing to d_hx, ds_self or ds_nbr.  With an
 * all-ones mask and no coef the results are bitwise those of uds_gat_backward. */
int uds_gat_backward_ex(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad, const float *hx,
                        const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr,
                        const float *edge_mask, const float *coef, int64_t S, int64_t d, float *alpha_ws, float *de_ws,
                        float *d_hx, float *ds_self, float *ds_nbr, uds_stream_t stream);

/* The whole reverse mode of a single-head GAT layer after its projection, as ONE operator: uds_gat_backward_ex with the
 * activation backward, the bias gradient and the attention-kernel gradients folded into its two passes (the tape through
 * GATConv of emulator.py:225-230 in the training step, emulator.py:457-484).  out (S,n,d) = the layer's output, gout = dL/dout,
 * act = the layer's UDS_ACT_* code; edge_mask / coef (S,nnz) or NULL as in uds_gat_backward_ex.
 *   g     = gout * act'(out)           in registers of the row pass, in fp32 with the operation order of the element-wise form
 *                                      (relu: out > 0 ? gout : 0; tanh: gout * (1 - out * out), no FMA; ...)
 *   d_hx, ds_self, ds_nbr              bitwise those of uds_gat_backward_ex on that g with an edge_mask, of uds_gat_backward[_coef]
 *                                      without one (the row pass takes the kernel those entries take)
 *   db (d,)    = sum_{s,i} g[s,i,:]                                                      or NULL: not computed
 *   da (2,d)   = [sum_{s,i} ds_self[s,i] hx[s,i,:], sum_{s,i} ds_nbr[s,i] hx[s,i,:]]     or NULL: not computed
 * db and da are summed in fp32: per thread over its rows, per workgroup over its threads in LDS, then over the workgroups'
 * partials by a third launch, each in a fixed order -- no atomics, the same inputs give the same bits.  Three launches: rows,
 * columns, reduce.  workspace: uds_gat_backward_act_workspace_floats(S, n, nnz, d) floats, 16-byte aligned, holding alpha and
 * de (S * nnz each), g (S * n * d) and the partials (3 * d * min(S * n, 2048) floats: a workgroup owns consecutive row blocks,
 * so their number does not grow with the batch); workspace_floats = its size.  Returns -22 and touches nothing for a NULL
 * argument, d not a multiple of 4 or above 256, S outside [0, 65535], a transposed handle of another shape or entry count, an
 * unknown activation code, misaligned tensors or a workspace that is too small.  S = 0 or an empty pattern: db = da = 0. */
int64_t uds_gat_backward_act_workspace_floats(int64_t S, int64_t n, int64_t nnz, int64_t d);
int uds_gat_backward_act(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *out, const float *gout, int act,
                         const float *hx, const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr,
                         const float *edge_mask, const float *coef, int64_t S, int64_t d, float *d_hx, float *ds_self,
                         float *ds_nbr, float *db, float *da, float *workspace, int64_t workspace_floats, uds_stream_t stream);

/* MULTI-HEAD attention / aggregation: spektral GATConv with attn_heads = H, concat_heads true or false and return_attn_coef
 * (GATConv._call_dense; the reference builds its layers with one head, emulator.py:229-230, so H > 1 is an extension of it).
 * hx (S, n, H*C) with head-major columns (x @ kernel.reshape(F, H*C)), s_self / s_nbr (S, n, H), edge_mask (S, nnz) or NULL shared
 * by the heads, coef (S, H, nnz) or NULL per head, both as in uds_gat_aggregate_ex.  Per head h
 *   pre[s,i,h,:] = sum_j alpha[s,h,i,j] coef[s,h,ij] hx[s,j,h*C:(h+1)*C],  alpha = softmax_j leaky_relu_0.2(s_self[s,i,h] + s_nbr[s,j,h]).
 * concat != 0: out (S, n, H*C) = act(pre + bias (H*C,)); concat == 0: out (S, n, C) = act(mean_h pre + bias (C,)).
 * alpha_out (S, H, nnz) or NULL receives alpha * coef of every entry of every head, 0 for a masked one: without coef the softmax
 * itself, which is what return_attn_coef returns.  C % 4 == 0, C <= 256.  With H == 1 and concat != 0 the result is bitwise that
 * of uds_gat_aggregate_ex. */
int uds_gat_aggregate_heads(const uds_csr_t *g, const float *hx, const float *s_self, const float *s_nbr, const float *bias,
                            const float *edge_mask, const float *coef, int64_t S, int64_t H, int64_t C, int concat, int act,
                            float *out, float *alpha_out, uds_stream_t stream);
/* Reverse mode of uds_gat_aggregate_heads (the tape through GATConv._call_dense with attn_heads = H).  grad = dL/dpre shaped like
 * `out` (for concat == 0 every head receives grad / H), a_self / a_nbr (H*C,) head-major, alpha_ws / de_ws S*H*nnz floats each,
 * d_hx (S, n, H*C), ds_self / ds_nbr (S, n, H).  A row pass and a column pass, no atomics: deterministic.  With H == 1 and
 * concat != 0 the results are bitwise those of uds_gat_backward_ex. */
int uds_gat_backward_heads(const uds_csr_t *g, const uds_csr_t *gt, const int32_t *perm_t, const float *grad, const float *hx,
                           const float *s_self, const float *s_nbr, const float *a_self, const float *a_nbr,
                           const float *edge_mask, const float *coef, int64_t S, int64_t H, int64_t C, int concat,
                           float *alpha_ws, float *de_ws, float *d_hx, float *ds_self, float *ds_nbr, uds_stream_t stream);

/* out[k] = sum_s <a[s, row(k), :], b[s, col(k), :]> for every entry k of the pattern (row-major order): the gradient
 * of the per-entry values of uds_csr_spmm (a = dL/dout (S,n_rows,F), b = x (S,n_cols,F)) -- NodeEdge.weight / bias
 * on the incidence support (emulator.py:34-45). */
int uds_csr_sddmm(const uds_csr_t *csr, const float *a, const float *b, int64_t S, int64_t F, float *out,
                  uds_stream_t stream);

/* Weight (and bias) gradient of a row GEMM / causal Conv1D tap on the matrix cores (split-bf16, 3 products):
 *   d_kernel[f, n] = sum_{b,t,r} a[b, t - shift, r, f] * g[b, t, r, n]   (terms with t < shift dropped),
 *   d_bias[n]      = sum_{b,t,r} g[b, t, r, n]                            (with_bias != 0),
 * a:(B,T,R,F), g:(B,T,R,H), F + (with_bias != 0) <= 128 and H <= 64 (uds_wgrad_workspace_floats() == 0 otherwise).
 * Dense layers: T = 1, shift = 0.  Deterministic (no atomics).  workspace: uds_wgrad_workspace_floats() floats.
 * Replaces the tape's `X^T dZ` products of emulator.py:457-484 (a library GEMM cannot split this reduction). */
int64_t uds_wgrad_workspace_floats(int64_t rows, int64_t F, int64_t H, int with_bias);
int uds_wgrad(const float *a, const float *g, int64_t B, int64_t T, int64_t R, int64_t F, int64_t H, int64_t shift,
              int with_bias, float *workspace, float *d_kernel, float *d_bias, uds_stream_t stream);

/* The same gradient for the wide layers of a default-size model (embed_size 128, GRU / LSTM projections of 192 / 256 columns):
 * every 1 <= F <= 256 and 1 <= H <= 256, with or without the bias row, widths that are no multiple of 16 and the shapes
 * uds_wgrad takes included.  Semantics, d_kernel's arithmetic (split-bf16, 3 products, fp32 accumulate) and refusals are
 * uds_wgrad's: terms with t < shift dropped, d_bias the column sum of g over ALL rows whatever the shift, B * T * R == 0 gives
 * zeros by memset, B * T * R < INT32_MAX, NULL arguments / with_bias without d_bias / non-positive sizes return -22; any other
 * F or H returns -22 too (message "uds_wgrad_wide: ...") and uds_wgrad_wide_workspace_floats() is 0 for it.  d_bias is summed
 * in plain fp32 from the g values the kernel holds anyway (no row of ones in a: at F = 128 and 256 it would open a tile row).
 * The output is cut into at most 2 x 4 blocks of at most 128 x 64; the (up to 8) waves of one workgroup each own a block
 * and walk the same rows together, so a and g are fetched from memory once per call.  One partial per workgroup in
 * `workspace` (uds_wgrad_wide_workspace_floats() floats, all of them written), summed in index order by a second launch:
 * no atomics, the same inputs give the same bits.  No allocation, no synchronisation. */
int64_t uds_wgrad_wide_workspace_floats(int64_t rows, int64_t F, int64_t H, int with_bias);
int uds_wgrad_wide(const float *a, const float *g, int64_t B, int64_t T, int64_t R, int64_t F, int64_t H, int64_t shift,
                   int with_bias, float *workspace, float *d_kernel, float *d_bias, uds_stream_t stream);

/* Parameter gradient of a dense-parameter NodeEdge, out[s] = (weight o inci + bias) @ x[s] (emulator.py:27-45 under the tape of
 * :457-484): d_bias[r, m] = sum_{s, k} g[s, r, k] x[s, m, k] and, when inci and d_weight are both given, d_weight = d_bias * inci
 * (one fp32 multiply per element).  g (S, R, h) and x (S, M, h) are read where they lie (h contiguous: the MFMA operands' own
 * layout), no permuted or transposed copy, no library.  Split-bf16 (hi + lo, three products, fp32 accumulate).  The output is cut
 * into 64 x 64 tiles and the reduction over S into pieces whose count depends on (R, M, S, h) alone; the partials
 * (uds_node_edge_wgrad_workspace_bytes() bytes of `workspace`, all of them written) are summed in a fixed order by a second
 * launch: no atomics, the same inputs give the same bits.  No allocation, no synchronisation.
 * Accepted: h % 4 == 0, 4 <= h <= 64 (an h that is no multiple of 32 is padded with zeros on chip), R, M >= 1, 0 <= S <= 2^24,
 * at most 2^20 tiles; g and x 16-byte aligned.  S == 0 writes zeros.  Anything else, a NULL d_bias, or d_weight without inci
 * returns -22, launches nothing and leaves the outputs untouched; the workspace size is then 0.
 * uds_node_edge_wgrad_plan is host only (works without a GPU): info4 = {k-steps of 32 per snapshot = the instantiation
 * k_node_edge_wgrad<1 | 2>, 0 when the shape is refused; pieces; snapshots per piece; 1 when h is padded}. */
int uds_node_edge_wgrad_plan(int64_t R, int64_t M, int64_t S, int64_t h, int32_t *info4);
int64_t uds_node_edge_wgrad_workspace_bytes(int64_t R, int64_t M, int64_t S, int64_t h);
int uds_node_edge_wgrad(const float *g, const float *x, int64_t S, int64_t R, int64_t M, int64_t h, const float *inci,
                        void *workspace, float *d_bias, float *d_weight, uds_stream_t stream);

/* ---- one spatial layer (node side + link side) ---------------------------------------------- */
typedef struct uds_network uds_network_t;

/* Borrows the four patterns (they must outlive the network): adj (N x N) and edge_adj (E x E) with
 * self loops, inc_n (N x E) node<-links incidence support, inc_e (E x N) its transpose. */
int uds_network_create(const uds_csr_t *adj, const uds_csr_t *edge_adj, const uds_csr_t *inc_n,
                       const uds_csr_t *inc_e, uds_network_t **out);
int uds_network_destroy(uds_network_t *net);
/* uds_network_create plans the fused kernel for 64-wide node and link rows.  Layers with 96-wide inputs (the first
 * layer of block 2: H + d/2 features, emulator.py:260-262) need their own tile plans: build them here, once, before
 * the first forward with those widths (allocates; afterwards forwards stay allocation-free).  Without it such a layer
 * runs the unfused kernels.  fx / fe = input widths of the node / link side. */
int uds_network_prepare(uds_network_t *net, int64_t fx, int64_t fe);
/* info8 = {fused plan available, node tiles, link tiles, max primary rows per tile, max secondary rows per
 * tile, max metadata ints per tile, LDS bytes per workgroup, t_node*1000 + t_link}.
 * info8[0] is a bit set over the plans built so far: 1 = <64,64>, 2 = <64,96> and <96,64>, 4 = <96,96>, 8 = <128,128>,
 * 16 = <128,64> and <64,128>, 32 = the <64,64> plan also fits the wave-specialised d = 64 kernel, the only d = 64 kernel
 * that takes a remainder (uds_spatial_layer_forward_rem refuses a 64 / 64 layer on a network without this bit). */
int uds_network_plan_info(const uds_network_t *net, int32_t *info8);

/* Host-only access to the tile planner (integer bookkeeping; works without a GPU).  A plan clusters the
 * primary rows of each side (nodes under adj, links under edge_adj) into tiles of at most t_node / t_link
 * rows (clusters whose primary / secondary footprint exceeds p_limit / q_limit > 0 are bisected) and lists, per
 * tile, own rows, halo rows, secondary rows and local CSR indices (layout:
 * gnn_uds_amd/csrc/tile_plan.hpp).  hdr_out holds 8 ints per tile, pool_out pool_len ints. */
typedef struct uds_tile_plan uds_tile_plan_t;
int uds_tile_plan_create(const int32_t *adj_rowptr, const int32_t *adj_col, const int32_t *eadj_rowptr,
                         const int32_t *eadj_col, const int32_t *incn_rowptr, const int32_t *incn_col,
                         const int32_t *ince_rowptr, const int32_t *ince_col, int64_t n_node,
                         int64_t n_edge, int32_t t_node, int32_t t_link, int32_t p_limit,
                         int32_t q_limit, uds_tile_plan_t **out);
int uds_tile_plan_destroy(uds_tile_plan_t *plan);
int uds_tile_plan_sizes(const uds_tile_plan_t *plan, int64_t *n_tiles, int64_t *pool_len, int32_t *caps3);
int uds_tile_plan_copy(const uds_tile_plan_t *plan, int32_t *hdr_out, int32_t *pool_out);
/* What the row-by-row refinement of the plan did, both sides together (tile_plan.hpp: TileRefiner): counts3 = rows a
 * fuller tile absorbed at no cost (fill), rows moved to shrink a halo (move), tiles dissolved into their neighbours. */
int uds_tile_plan_refine_counts(const uds_tile_plan_t *plan, int64_t *counts3);
/* The tile blocks the fused d = 64 kernel fetches (host-only, integer bookkeeping): one block per tile of the merged
 * list at a fixed stride of *stride_out ints, [8-int header | fixed-width index lists] (layout:
 * gnn_uds_amd/csrc/tile_plan.hpp, "Tile blocks of k_fused_tile").  Pass blocks_out = NULL to query the stride.  Returns
 * UDS_EINVAL when a tile exceeds the byte-wide local indices (255 primary / 256 secondary rows). */
int uds_tile_plan_blocks(const uds_tile_plan_t *plan, int32_t *blocks_out, int64_t *stride_out);

typedef struct uds_spatial_params {
  const float *xe_k, *xe_b; /* Dense(h) on e -> x_e : (fe, h), (h)            emulator.py:225 */
  const float *ex_k, *ex_b; /* Dense(h) on x -> e_x : (fx, h), (h)            emulator.py:226 */
  const float *ne_n_val;    /* NodeEdge(|inci|)   on its support: nnz(inc_n)  emulator.py:227 */
  const float *ne_e_val;    /* NodeEdge(|inci|^T) on its support: nnz(inc_e)  emulator.py:228 */
  const float *gx_k, *gx_as, *gx_an, *gx_b; /* GAT nodes: (fx+h, d),(d),(d),(d) emulator.py:229 */
  const float *ge_k, *ge_as, *ge_an, *ge_b; /* GAT links: (fe+h, d),(d),(d),(d) emulator.py:230 */
  const void *packed;       /* optional: output of uds_spatial_pack_weights for THESE kernels (device, 16-B aligned);
                               NULL = pack inside every forward call (4 tiny launches) */
} uds_spatial_params_t;

/* Bytes of the packed-weight buffer (fixed, covers fx, fe up to 96). */
int64_t uds_spatial_packed_bytes(void);
/* Splits the four kernels xe_k, ex_k, gx_k, ge_k into bf16 hi/lo MFMA fragments for the fused kernel.  Call once per
 * parameter update; the buffer must outlive the forward calls that reference it. */
int uds_spatial_pack_weights(const uds_spatial_params_t *params, int64_t fx, int64_t fe, int64_t h, int64_t d,
                             void *packed_out, uds_stream_t stream);

/* flags of uds_spatial_layer_forward */
enum {
  UDS_FLAG_EXACT_FP32 = 1,   /* exact-fp32 fmaf kernels (unfused); default is the fused kernel whose GEMMs
                                run as 3-term bf16-split MFMA with fp32 accumulation (~2^-16 per product) */
  UDS_FLAG_REQUIRE_FUSED = 2 /* fail instead of falling back when the fused kernel cannot take the shape */
};

/* Floats of workspace uds_spatial_layer_forward needs. */
int64_t uds_spatial_workspace_floats(const uds_network_t *net, int64_t S, int64_t h, int64_t d);

/* x:(S,N,fx), e:(S,E,fe) -> out_x:(S,N,d), out_e:(S,E,d).  out_* must not alias x / e.
 * Fused single-pass kernel for h = 32, d = 64, fx, fe in {64, 96}; other shapes (and UDS_FLAG_EXACT_FP32)
 * run the unfused exact-fp32 kernels. */
int uds_spatial_layer_forward(const uds_network_t *net, const uds_spatial_params_t *params,
                              const float *x, int64_t fx, const float *e, int64_t fe, int64_t S,
                              int64_t h, int64_t d, int act, int flags, float *workspace,
                              float *out_x, float *out_e, uds_stream_t stream);

/* The same layer with 96-wide inputs given as TWO tensors each: x = [xa (S,N,64) | xb (S,N,32)], e likewise (xb / eb
 * NULL with fxb / feb 0 = a single tensor).  The reference concatenates the boundary / action embeddings to the
 * temporal outputs before block 2 (emulator.py:260-262); here the concatenation is never materialised: the kernel
 * fetches a row's two pieces from the two tensors.  Fused kernel only (h = 32, d = 64). */
int uds_spatial_layer_forward_split(const uds_network_t *net, const uds_spatial_params_t *params, const float *xa,
                                    int64_t fxa, const float *xb, int64_t fxb, const float *ea, int64_t fea,
                                    const float *eb, int64_t feb, int64_t S, int64_t h, int64_t d, int act, int flags,
                                    float *workspace, float *out_x, float *out_e, uds_stream_t stream);

/* The same layer for a TRAINED NodeEdge: h = 64, d = 128, fx = 128, fe = 128 or 64 (the reference's default width) or h = 32,
 * d = 64, fx = fe = 64.  The reference's layer is matmul(w * inci + b, x) with a dense trainable b (emulator.py:36-45): after
 * training b is non-zero off the incidence support, and that part, rem_x = (b_n off the support) @ Dense_xe(e) (S,N,h) and
 * rem_e = (b_e off the support) @ Dense_ex(x) (S,E,h), is a dense GEMM (uds_remainder_forward).  Here it is added to the
 * support aggregate inside the fused kernel (one h-float row per primary row and snapshot, prefetched one snapshot ahead).
 * Fused kernel only: UDS_EINVAL when the shape or the network's tile plan does not take it. */
int uds_spatial_layer_forward_rem(const uds_network_t *net, const uds_spatial_params_t *params, const float *x, int64_t fx,
                                  const float *e, int64_t fe, const float *rem_x, const float *rem_e, int64_t S, int64_t h,
                                  int64_t d, int act, int flags, float *workspace, float *out_x, float *out_e,
                                  uds_stream_t stream);

/* keras.optimizers.Adam(learning_rate, beta_1, beta_2, epsilon, clipnorm) as TF 2.10 applies it (emulator.py:111), on a whole
 * list of tensors with the step count on the device -- nothing per step is computed on the host, so a captured graph replays it:
 *   n_i = ||g_i||_2;  g_i *= clipnorm / max(n_i, clipnorm) (per tensor; clipnorm <= 0: no clipping);
 *   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= lr_t m / (sqrt(v) + eps),  lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) (in double),
 *   t = state[0] + 1.
 * tensors: a HOST array of n_tensors records of DEVICE pointers (contiguous fp32, 4-byte aligned: 16-byte alignment and a length
 * that is a multiple of 4 are used where present, not assumed; numel = 0 records are skipped).  The records are copied into the
 * kernel arguments (64 tensors per launch): the array may be freed when the call returns.  g is only read.
 * loss: one device float or NULL.  state: int32[4] on the device, zero before the first call: [0] t, [1] status of this call
 * (bit 0: *loss is NaN / Inf, bit 1: some gradient element is NaN / Inf, i.e. a gradient norm is not finite), [2], [3] scratch.
 * With a status bit set the call changes none of p, m, v, t.  Otherwise t becomes t + 1, also when n_tensors = 0.
 * Two passes over the same workgroups (one per 4096 elements of a tensor): sums of squares in double into the workspace, then
 * the tensor's partials added in index order and the update; no atomics (two calls on the same inputs give the same bits), no
 * allocation, no copy, no synchronisation.  workspace: uds_adam_workspace_floats(numel, n_tensors) floats, 8-byte aligned. */
typedef struct {
  float *p;
  const float *g;
  float *m;
  float *v;
  int64_t numel;
} uds_adam_tensor_t;
int64_t uds_adam_workspace_floats(const int64_t *numel, int64_t n_tensors);   /* HOST array; -1 on a bad argument */
int uds_adam_step(const uds_adam_tensor_t *tensors, int64_t n_tensors, const float *loss, double lr, double beta_1, double beta_2,
                  double epsilon, double clipnorm, int32_t *state, float *workspace, int64_t workspace_floats, uds_stream_t stream);

/* A training batch of sliding windows on the device.  The reference builds every training batch on the host: sliding windows cut from the event series
 * (dataloader.py:93-95,144-169), one random batch of them per epoch (DataGenerator.prepare_batch, dataloader.py:106-143), five
 * normalisations and the uploads (main.py:209-232).  Here the series stay on the device, time-major, all events concatenated
 * into Ttot rows: states (Ttot, N, 4) = [h, q_totin, q_ds, r], flood (Ttot, N) >= 0, edge_states (Ttot, E, 4) = [depth, volume,
 * flow, setting], settings (Ttot, n_act) or NULL (n_act = 0), tide (Ttot, N) or NULL.
 *
 * uds_window_batch fills the six tensors of B windows in ONE launch.  The window at start s = starts[w] (device int32) covers
 * rows s .. s + seq_in + t_out - 1; with cx = if_flood ? 5 : 4 and cb = tide ? 2 : 1:
 *   x  (B, seq_in, N, cx)  row s + t:           [h, q_totin - r, q_ds, (flood > 0 ? 1 : 0, with if_flood), r]
 *   b  (B, t_out, N, cb)   row s + seq_in + t:  [r, (tide)]
 *   y  (B, t_out, N, cx)   row s + seq_in + t:  [h, q_totin - r, q_ds, (flood bit), flood]
 *   ex (B, seq_in, E, 4)   row s + t            ey (B, t_out, E, 3)  row s + seq_in + t, the first three link channels
 *   a  (B, t_out, n_act)   row s + seq_in + t of settings, never normalised (NULL exactly when n_act = 0)
 * norm (NULL = everything raw): device (span, min) pairs, span = max - min formed by the caller: x (N, cx), b (N, cb), y (N, cx),
 * e (E, 4) (ey uses its first three channels); a NULL pair leaves that tensor raw.  Each value becomes (v - min) / span with a
 * correctly rounded division (Emulator.normalize).  A window with s < 0 or s + seq_in + t_out > Ttot reads nothing and gets
 * EVERY output element set to NaN -- starts are device values the host cannot check; whether a window stays inside one event
 * is the caller's business.  Series and outputs 16-byte aligned; all offsets are 64-bit.  No allocation, no copy, no
 * synchronisation, no host read of a device value (safe inside a stream capture). */
typedef struct {
  const float *states, *flood, *edge_states, *settings, *tide;
  int64_t Ttot, N, E, n_act;
} uds_window_series_t;
typedef struct {
  const float *span_x, *min_x, *span_b, *min_b, *span_y, *min_y, *span_e, *min_e;
} uds_window_norm_t;
int uds_window_batch(const uds_window_series_t *series, const uds_window_norm_t *norm, const int32_t *starts, int64_t B, int64_t seq_in,
                     int64_t t_out, int if_flood, float *x, float *a, float *b, float *y, float *ex, float *ey, uds_stream_t stream);

/* The random batch of DataGenerator.prepare_batch (dataloader.py:106-143, over the windows of dataloader.py:93-95,144-169; one
 * draw per epoch and table in main.py:209-232), on the device: B (1 .. 4096) starts from a table of W windows with integer
 * weights.  Draw i of the call has the index j = *count + i and takes Philox4x32-10 (as uds_dropout) with key = seed, counter =
 * (j, 0), r = word0 << 32 | word1, u = (r * total) >> 64 with total = cum[W - 1]; out[i] = starts_table[k] for the smallest k
 * with cum[k] > u (cum: the inclusive 64-bit prefix sums of the weights, device).  A second one-thread launch on the same stream
 * then sets *count += B (count: one device uint64), so no thread reads count after it moved.  All integer arithmetic.  No
 * allocation, no copy, no synchronisation, no host read of a device value (safe inside a stream capture). */
int uds_window_draw(const int32_t *starts_table, const uint64_t *cum, int64_t W, int64_t B, uint64_t seed, uint64_t *count, int32_t *out,
                    uds_stream_t stream);

/* Model-predictive control on the device (gnn_uds_amd/mpc.py: Problem).
 *
 * uds_mpc_objective: the scenario objective (objective_pred_tf, envs/scenario/astlingen.py:75-99) of pop predicted horizons,
 * preds (pop, T, N, C) with q_w = channel C - 1 (flooding volume) and q_in = channel 1 (inflow):
 *   obj[p] = sum_t gamma[t] sum_n ( w_flood[n] q_w[p,t,n] + w_out[n] q_in[p,t,n] + w_smooth[n] |q_in[p,t,n] - q_in[p,t-1,n]| ),
 *   q_in[p,-1,n] = q_in0[p * q0_stride + n]: the inflow of the last history step, q0_stride = 0 (one row (N) shared by the
 *   population) or N (one row per candidate).
 * w_flood / w_out / w_smooth: (N) weights, the index / weight lists of the targets scattered into dense vectors (duplicate
 * indices summed); a NULL vector is an absent term, at least one is given.  A term whose weight is 0 is not formed and its
 * channel not read.  gamma: (T) or NULL (= ones).  Limits: C in [2, 8], T in [1, 4096], N in [1, 2^24], pop in [0, 2^20]
 * (pop = 0: nothing launched).  One workgroup per candidate, fp64 sums in one fixed order, no atomics: a second call gives
 * the same bits, and |obj - exact| <= 2 * 2^-24 * sum|term| (csrc/kernels_mpc.hpp derives it).
 *
 * uds_mpc_objective_backward: d_preds (pop, T, N, C) = the gradient of sum_p g[p] obj[p]; EVERY element is written, 0 where no
 * weight reaches.  The sub-gradient of |.| at 0 is 0 (torch.abs).  Each element is its contributions summed in fp64 and rounded
 * once.  q_in0 gets no gradient (it is history).
 *
 * Both: every pointer 16-byte aligned; no allocation, no copy, no synchronisation (safe inside a stream capture). */
int uds_mpc_objective(const float *preds, const float *q_in0, int64_t q0_stride, int64_t pop, int64_t T, int64_t N, int64_t C, const float *w_flood,
                      const float *w_out, const float *w_smooth, const float *gamma, float *obj, uds_stream_t stream);
int uds_mpc_objective_backward(const float *preds, const float *q_in0, int64_t q0_stride, const float *g, int64_t pop, int64_t T, int64_t N, int64_t C,
                               const float *w_flood, const float *w_out, const float *w_smooth, const float *gamma, float *d_preds,
                               uds_stream_t stream);

/* The cross-entropy method over decision vectors in [0, 1]^n_var.  The sampling and update rules are this project's own (the
 * reference's run_ce is a host loop over a TensorFlow model); pop in [2, 1024], n_var in [1, 1024], every pointer 16-byte
 * aligned, no allocation, no copy, no synchronisation, no host read of a device value.
 *
 * uds_ce_draw: out (pop, n_var).  Candidate i of the call has the index j = *count + i; variable v takes Philox4x32-10 (as
 * uds_dropout) with key = seed and counter = (j, v) -> words w0, w1;  u1 = ((w0 >> 8) + 0.5) 2^-24, u2 = ((w1 >> 8) + 0.5) 2^-24,
 * evaluated in fp32 (the sum k + 0.5 is exact for k < 2^23 and rounds to even above, so u lies in (0, 1]);
 *   z = sqrtf(-2 logf(u1)) cosf(2 pi u2),   out[i, v] = min(max(mean[v] + std[v] z, 0), 1).
 * A second one-thread launch on the same stream then sets *count += pop (count: one device uint64), so no thread reads count
 * after it moved: two calls of pop rows draw what one call of 2 pop rows draws.
 *
 * uds_ce_update: y (pop, n_var) the candidates, obj (pop) their objectives.  key(p) = obj[p], any NaN / Inf taken as +inf;
 * rank(p) = #{q: key(q) < key(p) or (key(q) == key(p) and q < p)} (integer comparisons); p is elite when rank(p) < n_elite
 * (1 <= n_elite <= pop) and obj[p] is finite.  Over the K elites, per variable: m = mean, s = population standard deviation
 * (two passes, ddof 0), both as balanced trees of 10 levels in rank order;
 *   mean <- smooth mean + (1 - smooth) m,   std <- max(smooth std + (1 - smooth) s, std_min)      (smooth in [0, 1]).
 * best_y (n_var) / best_obj (1) take the rank-0 candidate when it is finite and obj < *best_obj (start best_obj at +inf).
 * K = 0: mean, std, best_y and best_obj stay and status[0] = 1; status[0] is never cleared here (the caller zeroes it before
 * its loop and reads it once after).  best_obj and status are written by a second launch on the same stream. */
int uds_ce_draw(const float *mean, const float *std, int64_t n_var, int64_t pop, uint64_t seed, uint64_t *count, float *out, uds_stream_t stream);
int uds_ce_update(const float *y, const float *obj, int64_t pop, int64_t n_var, int64_t n_elite, double smooth, double std_min, float *mean, float *std,
                  float *best_y, float *best_obj, int32_t *status, uds_stream_t stream);

/* Which launches a fused spatial layer makes (host-only bookkeeping: neither entry touches a device).
 *
 * The snapshots of a launch are cut into chunks and one workgroup handles one (tile, chunk) pair: *chunk = the chunk
 * length of a launch of S snapshots over working_tiles tiles (1 whenever S * working_tiles <= 256; the last chunk holds
 * the S % chunk left-over snapshots).  S, working_tiles in [1, 2^31). */
int uds_fused_chunk(int64_t S, int64_t working_tiles, int64_t *chunk);
/* kernels of the fused spatial layer */
enum {
  UDS_KERNEL_FUSED_WS = 1,   /* k_fused_ws: the wave-specialised d = 64 kernel, 64-wide rows on both sides */
  UDS_KERNEL_FUSED_TILE = 2, /* k_fused_tile<FP, FS>: d = 64, primary / secondary rows of FP / FS in {64, 96} floats */
  UDS_KERNEL_FUSED_CS = 3    /* k_fused_cs<128, FP, FS>: the column-split d = 128 kernel, FP / FS in {64, 128} */
};
/* The launches uds_spatial_layer_forward (flags 0, single-tensor or split inputs alike) makes on this network for a layer
 * with fx / fe-wide node / link rows, h = d / 2 and output width d, from the plans built so far (uds_network_prepare):
 * info11 = {n, then for each of the n launches: kernel (UDS_KERNEL_*), FP, FS, side mask (1 = node tiles, 2 = link tiles,
 * 3 = both), tiles of the launch}; n = 0 when the layer runs unfused, 1 when both sides share a variant, 2 (node tiles,
 * then link tiles) when fx != fe.  Entries past the n-th launch are 0.  The chunk length of a launch over S snapshots is
 * uds_fused_chunk(S, tiles).  The forward decides with the same code. */
int uds_network_fused_launches(const uds_network_t *net, int64_t fx, int64_t fe, int64_t d, int32_t *info11);

#ifdef __cplusplus
}
#endif
#endif /* UDS_HIP_H */
