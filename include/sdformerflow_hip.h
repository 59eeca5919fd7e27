/* sdformerflow_hip.h - C ABI of libsdformerflow_hip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the SDformerFlow forward hot path.  The reference is
 * pure Python; the only native code on its path is SpikingJelly's CuPy multi-step neuron kernel,
 * switched on with `functional.set_backend(model, "cupy", neurontype)` (reference
 * eval_DSEC_flow_SNN.py:118-119).  Every entry point below names the reference call it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *   - the library never allocates or frees device memory and never synchronises; all work is
 *     enqueued on `stream` (a hipStream_t passed as void*; NULL = the legacy default stream)
 *   - return value: 0 = launched, <0 = argument error detected before any launch
 *     (SDF_E_*), >0 = the hipError_t of the failed launch.  No C++ exception crosses the ABI.
 *   - spikes are {0,1}; `*_dtype` selects their storage: SDF_F32 (the reference's own format)
 *     or SDF_U8 (1 byte/spike, the operand format of the spike GEMM)
 */
#ifndef SDFORMERFLOW_HIP_H
#define SDFORMERFLOW_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDF_VERSION 107   /* round 6 (107): + sdf_switches_reload, sdf_launch_log / sdf_launch_log_read, SdfQkAttnDesc.rep_windows, SdfSpikeGemmDesc.zg_rep; the diagnostic SDF_* switches are read once, not per call.  106 / round 5: + sdf_ann_attn_block_fwd, sdf_ann_mlp_block_fwd, sdf_spike_deconv3x3s2_fwd, row-major digit planes in sdf_spike_gemm_fwd; 106: + sdf_linear_dw_fwd, sdf_ringed_rows_fwd, sdf_linear_train_fwd */

enum { SDF_F32 = 0, SDF_U8 = 1 };
enum { SDF_LIF = 0, SDF_PSN = 1, SDF_IF = 2 };
enum {
  SDF_E_NULL = -1,    /* required pointer is NULL            */
  SDF_E_SHAPE = -2,   /* size / divisibility requirement     */
  SDF_E_DTYPE = -3,   /* unknown dtype / kind selector       */
  SDF_E_ALIGN = -4    /* pointer or stride alignment         */
};

int sdf_version(void);

/* The library's diagnostic switches (the SDF_* environment variables listed in INTEGRATION.md's appendix: A/B and tuning overrides,
 * none needed in production) are read from the environment ONCE, at the first call that asks for one, into a read-only table - no
 * entry point calls getenv() on its per-call path.  A test harness that changes the environment between calls re-reads the table
 * with this call (not concurrently with other calls into the library).  No reference counterpart. */
void sdf_switches_reload(void);

/* Diagnostic per-launch log (round 6; off by default, one relaxed atomic load per launch while off).  sdf_launch_log(1) clears the
 * log and switches it on: every kernel launch of every entry point is then bracketed by two HIP events on its own stream and noted
 * with its kernel, grid and block; sdf_launch_log(0) switches it off.  sdf_launch_log_read synchronises with the recorded launches
 * and copies up to `max_records` records in launch order; returns the number of launches logged (may exceed max_records).
 * `workgroups * us / 256` = the CHIP time of a launch (compute units x time it can hold), the measure bench.py's `roofline.by_time`
 * reports beside the duration.  Not for use during stream capture (events).  No reference counterpart. */
typedef struct SdfLaunchRecord {
  char kernel[192];         /* demangled kernel name with its template arguments */
  uint32_t workgroups, threads, lds_bytes;   /* grid size in workgroups, threads per workgroup, dynamic LDS bytes */
  float us;                 /* duration between the two events around the launch; -1: unavailable */
} SdfLaunchRecord;
void sdf_launch_log(int enable);
int sdf_launch_log_read(SdfLaunchRecord* out, int max_records);

/* ---------------------------------------------------------------------------------------------
 * Multi-step LIF over the leading (time) axis of a contiguous fp32 (T, N) tensor.
 * Replaces: neuron.LIFNode multi-step forward (reference Spiking_modules.py:40-47,98-99; the
 * CuPy backend of eval_DSEC_flow_SNN.py:118-119).  Arithmetic (each op separately rounded):
 *   h = v + (x_t - v)/tau ; s = (h - v_th >= 0) ; v = h - s*v_th (soft) | (1-s)*h + s*v_reset
 *   tau > 1: spikingjelly LIFNode.  0 < tau < 1 (every forward entry point and descriptor that carries a neuron): the
 *   multiplicative charge h = v + (x_t - v)*tau of ParametricLIFNode, tau = sigmoid(w) (reference Spiking_modules.py:75-82).
 *   tau <= 0 or tau == 1: SDF_E_SHAPE.  The backward entry points take tau > 1 only (PLIF: sdf_plif_bwd, below).
 * v starts at 0 (soft) or v_reset (hard).  `v_last` (fp32, N) receives the final membrane or is NULL.
 */
int sdf_lif_fwd(const float* x, void* spike, float* v_last, int T, int64_t N, float tau, float v_th,
                int soft_reset, float v_reset, int spike_dtype, void* stream);

/* Parallel Spiking Neuron: H = b + W X over time, S = (H >= 0).
 * Replaces: PSN.forward (reference Spiking_submodules.py:207-211).  H[t] is the fp32 fmaf chain
 *   h = b[t]; for k = 0..T-1: h = fmaf(W[t,k], x[k], h)
 * (an order the oracle restates exactly; torch.addmm's own order is BLAS-defined).
 * W is (T,T) row-major fp32, b is (T) fp32, both device memory.  T <= 32.
 */
int sdf_psn_fwd(const float* x, const float* W, const float* b, void* spike, int T, int64_t N,
                int spike_dtype, void* stream);

/* ---- training path: backward of the neurons -------------------------------------------------
 * Replaces: autograd through spikingjelly's multi-step LIFNode / IFNode (torch backend; the reference builds them in
 * Spiking_modules.py:40-66 with `surrogate_function=ATan()`, `detach_reset` from the YAML) - BPTT over the T steps:
 *   gh_t = gv_t * dv_t/dh_t + (gs_t [+ reset path unless detach_reset]) * g'(h_t - v_th)
 *   gx_t = gh_t / tau ;  gv_{t-1} = gh_t - gh_t / tau           (IF: gx_t = gv_{t-1} = gh_t)
 *   g'(u) = alpha/2 / (1 + (pi/2 * alpha * u)^2)                (surrogate.ATan, the only one the configs use)
 * x, grad_spike, grad_x: (T, N) fp32 contiguous, N % 4 == 0, 16-byte aligned.  The membrane trajectory is recomputed
 * from x with the forward's exact arithmetic - the forward saves nothing.  T in {1,2,4,5,8,10,16,20}.
 * Bit-equal to the CPU autograd of the reference formulas for detach_reset = 1. */
#define SDF_SURROGATE_ATAN 0
int sdf_lif_bwd(const float* x, const float* grad_spike, float* grad_x, int T, int64_t N, int kind, float tau,
                float v_th, int soft_reset, float v_reset, int detach_reset, int surrogate, float alpha, void* stream);

/* Backward of PSN.forward (reference Spiking_submodules.py:207-211): gh = grad_spike * g'(H), grad_x = W^T gh,
 * grad_W = gh X^T, grad_b = sum_n gh.  grad_W / grad_b (T*T, T fp32) are optional (both or neither, T <= 10): they are
 * reduced deterministically through `workspace` (sdf_psn_bwd_workspace_bytes, caller-owned).  grad_h (T, N) is an
 * optional copy of gh (for T > 10 form grad_W = grad_h X^T with a library GEMM). */
int64_t sdf_psn_bwd_workspace_bytes(int T, int64_t N);
int sdf_psn_bwd(const float* x, const float* W, const float* b, const float* grad_spike, float* grad_x, float* grad_W,
                float* grad_b, float* grad_h, void* workspace, int64_t workspace_bytes, int T, int64_t N, int surrogate,
                float alpha, void* stream);

/* Training path of ParametricLIFNode (spikingjelly; the reference's `neuron_type: plif`, Spiking_modules.py:75-82): the
 * multiplier k = sigmoid(w) is ONE fp32 in device memory (`plif_k`, the caller's sigmoid on the same stream), so a train step
 * reads nothing back to the host.  Forward: sdf_lif_fwd's arithmetic with tau = k (h = v + d * k, d = x - v or
 * x - (v - v_reset)), fp32 spikes, the same spikes eval mode gives for the same k.  Backward: sdf_lif_bwd's BPTT with
 *   gx_t = gh_t * k ;  gv_{t-1} = gh_t - gh_t * k ;  grad_k = sum_t sum_n gh_t * d_t      (k = 0.5: LIF tau = 2 bit for bit)
 * grad_k (one fp32) is reduced lane -> wave -> workgroup -> per-workgroup partials in `workspace`
 * (sdf_plif_bwd_workspace_bytes(T, N) = 4 * ceil(N / 1024) bytes, caller-owned) -> one fixed-order finish: no atomics, two calls
 * give bit-equal results.  Same shapes, T set and ATan surrogate as sdf_lif_bwd; soft / hard reset, any v_reset, detach_reset 0 / 1. */
int sdf_plif_fwd(const float* x, const float* plif_k, float* spike, int T, int64_t N, float v_th, int soft_reset, float v_reset,
                 void* stream);
int64_t sdf_plif_bwd_workspace_bytes(int T, int64_t N);
int sdf_plif_bwd(const float* x, const float* plif_k, const float* grad_spike, float* grad_x, float* grad_k, void* workspace,
                 int64_t workspace_bytes, int T, int64_t N, float v_th, int soft_reset, float v_reset, int detach_reset,
                 int surrogate, float alpha, void* stream);

/* Online gradient of SLTTLIFNode (the reference's `neuron_type: SLTTlif`, Spiking_submodules.py:11-90): the forward is sdf_lif_fwd;
 * the backward is sdf_lif_bwd's with the membrane detached between steps (:41), gv == 0 at every step:
 *   gx_t = grad_spike_t * g'(h_t - v_th) / tau
 * detach_reset has no effect (the reset only feeds the detached membrane), so the entry point does not take it.  Same shapes,
 * T set and trajectory recomputation as sdf_lif_bwd; tau > 1; a surrogate other than SDF_SURROGATE_ATAN returns SDF_E_SHAPE. */
int sdf_sltt_bwd(const float* x, const float* grad_spike, float* grad_x, int T, int64_t N, float tau, float v_th, int soft_reset,
                 float v_reset, int surrogate, float alpha, void* stream);

/* GLIF neuron (the reference's GatedLIFNode with layer-wise gates, `neuron_type: glif`, Spiking_submodules.py:94-181), forward and
 * BPTT.  `tab` = [L, Dk, g, R, th, c_0 .. c_{T-1}], 5 + T fp32 in DEVICE memory, formed by the caller on the same stream from the
 * 7 + T gate logits (a = sigmoid(alpha), b = sigmoid(beta)):
 *   L = 1 - a (1 - sigmoid(tau))   Dk = (1 - a) sigmoid(linear_decay)   g = sigmoid(gamma)   R = (1 - g) sigmoid(v_subreset)
 *   th = sigmoid(v_threshold)      c_t = 1 - b (1 - sigmoid(conduct_t))
 * The host never reads it.  Forward, from v = 0, s = 0, every op separately rounded in the reference's order:
 *   u = (L v - Dk) + x_t c_t ;  u = u - ((L v) g) s - R s ;  s = (u - th >= 0) ;  v = u
 * x (T, N) fp32 contiguous, N % 4 == 0, 16-byte aligned; spikes fp32 or u8; T in {2, 4, 5, 10, 20}, otherwise SDF_E_SHAPE.
 * Backward (the spike is NOT detached between steps): the trajectory is recomputed from x, then for t = T-1 .. 0
 *   S_t = gs_t + gu_{t+1} (-(L v_t) g - R) ;  gu_t = gu_{t+1} (L - L g s_t) + g'(u_t - th) S_t ;  grad_x_t = gu_t c_t
 * grad_tab (5 + T fp32): dL = sum gu_t (v_{t-1} - v_{t-1} g s_{t-1}), dDk = -sum gu_t, dg = -sum gu_t L v_{t-1} s_{t-1},
 * dR = -sum gu_t s_{t-1}, dth = -sum g'(u_t - th) S_t, dc_t = sum_n gu_t x_t; reduced lane -> wave -> workgroup -> one row of
 * partials per workgroup in `workspace` (sdf_glif_bwd_workspace_bytes(T, N) = 4 (5 + T) ceil(N / 1024) bytes, caller-owned) -> one
 * fixed-order finish: no atomics, two calls give bit-equal results.  ATan surrogate only: another one returns SDF_E_SHAPE, as does
 * a workspace that is too small. */
int sdf_glif_fwd(const float* x, const float* tab, void* spike, int T, int64_t N, int spike_dtype, void* stream);
int64_t sdf_glif_bwd_workspace_bytes(int T, int64_t N);
int sdf_glif_bwd(const float* x, const float* tab, const float* grad_spike, float* grad_x, float* grad_tab, void* workspace,
                 int64_t workspace_bytes, int T, int64_t N, int surrogate, float alpha, void* stream);

/* Batch-statistics BatchNorm over the last dim of a channel-last (R, C) fp32 buffer, forward and backward (training form of
 * the SpikingNormLayer "BN": spikingjelly layer.BatchNorm2d multi-step -> nn.BatchNorm2d on the view the reference makes with
 * permute(0,1,4,2,3); Spiking_modules.py:101-146, Spiking_swin_transformer3D.py:172, 178, 673, 677, 714, 972) - no permute
 * copies.  forward: y = (x - mean) * invstd * w + b with batch mean / biased variance (fp64 sums), save_mean / save_invstd (C)
 * for the backward, running stats updated in place with momentum and the unbiased variance (pass NULL, NULL to skip).
 * backward: grad_bias = sum gy, grad_weight = sum gy * xhat, grad_x = (gy - gb/R - xhat * gw/R) * invstd * w.
 * C % 4 == 0; workspace: sdf_bn_train_workspace_bytes(R, C) bytes (8-byte aligned), caller-owned; deterministic reductions. */
int64_t sdf_bn_train_workspace_bytes(int64_t R, int C);
int sdf_bn_train_fwd(const float* x, const float* weight, const float* bias, float* y, float* save_mean, float* save_invstd,
                     float* running_mean, float* running_var, int64_t R, int C, float eps, float momentum, void* workspace,
                     int64_t workspace_bytes, void* stream);
int sdf_bn_train_bwd(const float* x, const float* grad_y, const float* weight, const float* save_mean, const float* save_invstd,
                     float* grad_x, float* grad_weight, float* grad_bias, int64_t R, int C, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* The same for an NCHW buffer (N, C, H, W), HW = H * W a multiple of 4, C <= 2048: the conv outputs of the patch embedding
 * and the U-Net tail (layer.BatchNorm2d on (T*B, C, H, W), Spiking_modules.py:118, :291-296, :339-347, :467-474, :811-819,
 * :906-933).  Same statistics / outputs / workspace size as the channel-last pair. */
int sdf_bn_train_nchw_fwd(const float* x, const float* weight, const float* bias, float* y, float* save_mean, float* save_invstd,
                          float* running_mean, float* running_var, int64_t N, int C, int HW, float eps, float momentum,
                          void* workspace, int64_t workspace_bytes, void* stream);
int sdf_bn_train_nchw_bwd(const float* x, const float* grad_y, const float* weight, const float* save_mean,
                          const float* save_invstd, float* grad_x, float* grad_weight, float* grad_bias, int64_t N, int C, int HW,
                          void* workspace, int64_t workspace_bytes, void* stream);

/* Token gate of Spiking_QK_WindowAttention3D for the training path (reference Spiking_swin_transformer3D.py:687-694:
 * `q.sum(-1)` over each head's 32 channels -> sn2_q over the T' steps -> `k.mul(...)`), fp32 spike tensors (T', rows, C):
 *   forward   e = k * A,  A = SN2_q(head sums of q)
 *   backward  grad_k = grad_e * A ;  grad_q = BPTT of SN2_q applied to sum_d(grad_e * k), broadcast over the head's channels
 * LIF / IF / PSN gates (ATan surrogate; detach_reset as in sdf_lif_bwd); T' in {1, 2, 4}; C % 32 == 0; 16-byte aligned pointers.
 * PSN: psn_w (T',T') / psn_b (T') in, grad_psn_w / grad_psn_b out, reduced deterministically through `workspace`
 * (sdf_qk_gate_bwd_workspace_bytes); all five NULL otherwise.
 * One launch each instead of the ~8 elementwise / reduction launches autograd runs for the composed expression. */
int sdf_qk_gate_f32_fwd(const float* q, const float* k, float* e, int Tq, int64_t rows, int C, int kind, float tau, float v_th,
                        int soft_reset, float v_reset, const float* psn_w, const float* psn_b, void* stream);
int64_t sdf_qk_gate_bwd_workspace_bytes(int Tq, int64_t rows, int C);
int sdf_qk_gate_bwd(const float* q, const float* k, const float* grad_e, float* grad_q, float* grad_k, int Tq, int64_t rows, int C,
                    int kind, float tau, float v_th, int soft_reset, float v_reset, int detach_reset, int surrogate, float alpha,
                    const float* psn_w, const float* psn_b, float* grad_psn_w, float* grad_psn_b, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* The same gate with a PLIF SN2_q (ParametricLIFNode, the gate `Spiking_neuron` builds for `neuron_type: plif`, reference
 * Spiking_swin_transformer3D.py:636): the multiplicative charge with k = sigmoid(w) read from `plif_k` (one fp32, device memory).
 * The backward also returns grad_plif_k = sum over (t, row, head) of gh * d, reduced through `workspace`
 * (sdf_qk_gate_plif_bwd_workspace_bytes(Tq, rows, C) = 4 * ceil(rows * C / 1024) bytes) in a fixed order: bit-reproducible. */
int sdf_qk_gate_plif_f32_fwd(const float* q, const float* k, float* e, const float* plif_k, int Tq, int64_t rows, int C, float v_th,
                             int soft_reset, float v_reset, void* stream);
int64_t sdf_qk_gate_plif_bwd_workspace_bytes(int Tq, int64_t rows, int C);
int sdf_qk_gate_plif_bwd(const float* q, const float* k, const float* grad_e, float* grad_q, float* grad_k, const float* plif_k,
                         float* grad_plif_k, void* workspace, int64_t workspace_bytes, int Tq, int64_t rows, int C, float v_th,
                         int soft_reset, float v_reset, int detach_reset, int surrogate, float alpha, void* stream);

/* General neuron launch: strided / gathered input, fused eval-BatchNorm and additive prologue.
 * Replaces the reference idiom  SN( BN( y.permute(..) ).permute(..) [+ positional_encoding] )
 * (Spiking_swin_transformer3D.py:670-680, 168-174, 970) and the pad / roll / window_partition_v2
 * gather in front of it (:789-804), without materialising any of the permutes.
 *
 * One time step holds nb*ni logical elements; element (b, r) of step t lives at
 *     x   + b*x_sb + t*x_st + r          (dense mode,  rowmap == NULL)
 *     x   + rowmap[t*rows + row]*rowlen + col ,  row = (b*ni + r)/rowlen, col = (b*ni+r)%rowlen,
 *           rows = nb*ni/rowlen, a negative map entry reads as 0.0      (gather mode)
 *     out + b*o_sb + t*o_st + r
 * Prologue (in this order, all optional):  y = fmaf(x, alpha[c], beta[c]) with c = (r/inner) % C;
 *     y = y + add[t*add_st + r % add_period].
 * ni, all strides, rowlen, inner*C-blocks and add_period must be multiples of 4 unless inner == 1
 * is replaced by C % 4 == 0 (the kernel moves 4 elements per lane).
 */
typedef struct SdfNeuronDesc {
  const float* x;
  void* out;
  float* v_last;            /* LIF/IF only, dense (nb*ni) or NULL */
  int32_t T;
  int32_t out_dtype;        /* SDF_F32 | SDF_U8 */
  int64_t nb, ni;
  int64_t x_sb, x_st;
  int64_t o_sb, o_st;
  const int32_t* rowmap;    /* NULL = dense */
  int32_t rowlen;
  int32_t kind;             /* SDF_LIF | SDF_PSN | SDF_IF */
  const float* alpha;       /* NULL = no affine */
  const float* beta;
  int32_t C;
  int32_t inner;
  const float* add;         /* NULL = none */
  int64_t add_st, add_period;
  float tau, v_th, v_reset;
  int32_t soft_reset;
  const float* psn_w;       /* (T,T) */
  const float* psn_b;       /* (T)   */
  /* round 6: an outermost dimension - nrep > 1 equally laid out problems (dense mode only), problem p at x + p*x_srep / out + p*o_srep
   * (v_last dense over all nrep*nb*ni): the batch elements of a pixel-strided channel slice in one descriptor.  0 / 1 = none. */
  int64_t nrep, x_srep, o_srep;
} SdfNeuronDesc;

int sdf_neuron_fwd(const SdfNeuronDesc* d, void* stream);
/* n independent neuron calls as ONE launch when they share T in {2, 4, 5, 10, 20} and n <= 6 (otherwise one launch each): the
 * U-Net decoders' skip inputs - four small tensors that each paid a launch of their own (reference Spiking_modules.py:467-474). */
int sdf_neuron_multi_fwd(const SdfNeuronDesc* descs, int n, void* stream);
/* The general launch with the GLIF recurrence (the reference's GatedLIFNode, sdf_glif_fwd's arithmetic from v = 0, s = 0): the addressing
 * contract of sdf_neuron_fwd field for field - dense strides, rowmap gather, alpha / beta, add, nrep, out_dtype - and `tab` =
 * [L, Dk, g, R, th, c_0 .. c_{T-1}] in DEVICE memory as sdf_glif_fwd takes it.  kind, tau, v_th, v_reset, soft_reset and psn_* are not
 * read; v_last must be NULL and T in {2, 4, 5, 10, 20} (SDF_E_SHAPE), tab not NULL (SDF_E_NULL); every other check, and their order,
 * are sdf_neuron_fwd's.  What an eval forward of a GLIF model launches at every neuron call (no fused epilogue has a GLIF form). */
int sdf_glif_neuron_fwd(const SdfNeuronDesc* d, const float* tab, void* stream);
/* The general launch that also keeps the membrane (the reference's `store_v_seq = True`, eval_DSEC_flow_SNN.py:145-149, `vis.monitor_v`):
 * sdf_neuron_fwd's contract field for field - dense strides, rowmap gather with negative entries, alpha / beta with inner == 1 and
 * inner > 1, add, nrep, out_dtype, v_last, T in {2, 4, 5, 10, 20} compiled in and any other T at run time - and the same spikes bit for
 * bit, plus the membrane AFTER the reset of step t (spikingjelly's v_seq[t]) as fp32 at
 *     v_seq + b*o_sb + t*o_st + r        (+ p*o_srep for problem p of nrep)
 * i.e. `out`'s own addressing in fp32 elements: a v_seq tensor has the shape and strides of the spike tensor.  Nothing else of v_seq is
 * written.  Kinds SDF_LIF and SDF_IF; SDF_PSN has no membrane and is refused with SDF_E_DTYPE where the kind is checked.  v_seq NULL ->
 * SDF_E_NULL (with d), v_seq not 16-byte aligned -> SDF_E_ALIGN (behind the descriptor's own checks); every other check, and their
 * order, are sdf_neuron_fwd's.  Added to SDF_VERSION 107 (no existing entry changed). */
int sdf_neuron_vseq_fwd(const SdfNeuronDesc* d, float* v_seq, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spike GEMM:  out[M,N] = epilogue( A[M,K] (binary, u8) x W[N,K]^T ).
 * Replaces: sj_layer.Linear on spike tensors + the BatchNorm that follows it + the residual add
 * (reference Spiking_swin_transformer3D.py:170-178, 671-677, 712-714, 840, 845, 971-972).
 *
 * W is passed as `nsplit` bf16 planes (device, plane-major [nsplit][N][K]) with
 * W = plane0 + plane1 + plane2 (hi / mid / lo split made by sdf_split_weight_bf16); binary A is
 * exact in bf16, so nsplit = 3 reproduces the fp32 product to fp32 rounding on the bf16 MFMA path.
 * Epilogue, in order:  acc (+ bias[n]) ; fmaf(., alpha[n], beta[n]) if alpha ; (+ resid[row][n]) ;
 * stored fp32 at out[row*ldo + n] where row = out_rowmap ? out_rowmap[m] : m (negative = dropped)
 * and resid uses the same row.  `resid` may alias `out` (in-place residual update).
 *
 * A addressing: zg_nH == 0: A[m*lda + k].  zg_nH > 0: the reference's head-scramble
 *   Z[t,b,n,g*32+d] = E_flat[((((b*nH+g)*Tq+t)*N1+n)*32+d]   (Spiking_swin_transformer3D.py:709-710)
 * with m = (t*zg_B + b)*zg_N1 + n, k = g*32 + d, Tq = zg_T; requires K == nH*32.
 * zg_rep > 0 (round 6): the zg_B windows are zg_B / zg_rep INDEPENDENT problems of zg_rep windows each - replica r owns windows
 * r*zg_rep .. and its E_flat is the (Tq, zg_rep, N1, C) sub-tensor of the (Tq, zg_B, N1, C) buffer at those windows - so that one
 * launch sequence serves several batch-1 forwards with the reference's batch-1 semantics each (zg_rep % Tq == 0, zg_B % zg_rep == 0).
 * Requirements: K % 32 == 0, N % 32 == 0, lda % 16 == 0.
 */
typedef struct SdfSpikeGemmDesc {
  const uint8_t* A;
  const uint16_t* Wp;       /* bf16 bits, [nsplit][N][K] */
  float* out;
  int64_t M;
  int32_t N, K;
  int64_t lda, ldo;
  int32_t nsplit;           /* 1: one bf16 plane; 2: two fp16 planes of wscale*W (22 bits); 3: three bf16 planes (24 bits) */
  const float* bias;        /* NULL ok */
  const float* alpha;       /* NULL ok */
  const float* beta;
  const float* resid;       /* NULL ok */
  const int32_t* out_rowmap;/* NULL ok */
  int32_t zg_nH, zg_T, zg_B, zg_N1;
  /* Fused neuron epilogue (sn_T > 0):  out_spike = SN_T( fmaf(acc, alpha, beta) [+ add] ), 1-byte spikes, the fp32
   * pre-activation never leaves the chip.  Replaces Linear -> BN -> [+ positional_encoding] -> Spiking_neuron
   * (reference Spiking_swin_transformer3D.py:170-174, 671-680).  The M = pos_count*sn_T rows are (position, t)
   * pairs: row(P, t) = (P / pos_inner)*pos_ostride + P % pos_inner + t*t_stride, used for A and out_spike alike
   * (MLP on a (B,D,HW,.) tensor: pos_inner = HW, pos_ostride = D*HW, t_stride = HW; attention (T',rows,.):
   * pos_inner = rows, t_stride = rows).  add is (sn_T, add_prows, N) fp32 indexed [t][P % add_prows][n] or NULL.
   * sn_T in {2,4,5,10,20}; bias / resid / out_rowmap / zg_* must be unset; N % 16 == 0. */
  int32_t sn_T, sn_kind;    /* sn_T == 0: fp32 epilogue */
  float tau, v_th, v_reset;
  int32_t soft_reset;
  const float* psn_w;
  const float* psn_b;
  int64_t pos_count, pos_inner, pos_ostride, t_stride;
  const float* add;
  int64_t add_prows;
  uint8_t* out_spike;       /* (rows, N) u8 */
  /* Optional scratch for split-K (small M, large K): caller-owned device memory; when it holds at least
   * 2*M*N floats the library may run the product as K chunks + a deterministic k-ordered reduction. */
  void* workspace;
  int64_t workspace_bytes;
  /* nsplit == 2 only: 1 / wscale of the planes made by sdf_split_weight_f16x2 (a power of two); the accumulator is
   * multiplied by it - exactly - before the epilogue.  0 or 1 otherwise. */
  float acc_scale;
  /* With out_rowmap: number of rows of out / resid (an upper bound of the scattered row indices + 1); 0 = unknown.
   * Lets the library pick kernels that address the output with 32-bit offsets. */
  int64_t out_rows;
  /* nsplit == SDF_PLANES_I8X3 only: Wp is then int8_t[3][N][K] digit planes and col_scale[n] the power-of-two scale of output channel
   * n, both made by sdf_split_weight_i8x3: w[n][k] = (d2*65536 + d1*256 + d0) * col_scale[n].  NULL otherwise.  Taken by
   * sdf_spike_conv2d_fwd (3x3 / stride 1 / Cin 96 launches of the weight-resident convolution; the small-M convolution) and, since
   * round 5, by sdf_spike_gemm_fwd itself: a plain product with the fp32 epilogue (bias, alpha / beta, resid == out or NULL) on the
   * weight-resident row-loop kernel (csrc/ms_res.hip) for M % 10 == 0, K % 16 == 0, K <= 1024, lda == K - the stacked-tap products
   * of the middle decoder levels (reference Spiking_modules.py:461-474 as one product + sdf_deconv_col2im_fwd); SDF_E_SHAPE otherwise. */
  const float* col_scale;
  int32_t zg_rep;           /* head scramble: windows per independent replica (0 = zg_B: one problem) */
} SdfSpikeGemmDesc;

#define SDF_PLANES_I8X3 4
/* the same digits in MFMA fragment order (sdf_tile_weight_i8x3 below): what the small-M convolution kernel streams at full rate */
#define SDF_PLANES_I8X3_TILED 5

/* Weight-format helper for the 3x3 `layer.Conv2d` weights of MS_ResBlock / SEWResBlock (reference Spiking_modules.py:845-846,
 * 898-899; the reference has no counterpart - it multiplies fp32 weights with fp32 spike tensors in MIOpen / cuDNN).
 * fp32 weights (N, K) -> three int8 digit planes [3][N][K] + per-row power-of-two scales: q = rint(w / s) with
 * s = 2^(e - 23) with 2^e the power of two above max_k |w[n][k]| (23 bits + sign; 22 where the row maximum exceeds 0.996 * 2^e and the
 * top digit would leave int8), balanced base-256 digits.
 * Spikes are int8 values already: the spike x weight dot product becomes three exact int32 MFMA sums. */
int sdf_split_weight_i8x3(const float* W, int8_t* planes, float* col_scale, int N, int K, void* stream);

/* Digit planes [3][N][K] (sdf_split_weight_i8x3) -> fragment order [N / 16][K / 64][3][64][16 B]: the 1 KB a wave reads for one
 * 16-column x 64-deep x one-plane MFMA operand is contiguous and in lane order (lane l: column 16 j + l % 16, k = 64 s + 16 (l / 16) ..).
 * Same size as the planes; passed to sdf_spike_conv2d_fwd with nsplit = SDF_PLANES_I8X3_TILED and the same col_scale.  Only the
 * small-M kernels read it: the convolution (3x3 / stride 1, Cin % 64 == 0, at most 32 000 rows in (B, T, H, W) order: the U-Net
 * bottleneck of reference Spiking_modules.py:906-933) and, through sdf_spike_gemm_fwd with the same nsplit, the plain product with the
 * fp32 epilogue (M % 10 == 0, M <= 5 120, lda == K, K % 64 == 0, no out_rowmap / zg / add / neuron: the first decoder's stacked-tap GEMM,
 * reference Spiking_modules.py:461-474); other shapes return SDF_E_SHAPE.  N % 16 == 0, K % 64 == 0. */
int sdf_tile_weight_i8x3(const int8_t* planes, int8_t* tiled, int N, int K, void* stream);

int sdf_spike_gemm_fwd(const SdfSpikeGemmDesc* d, void* stream);

/* The plain form of the spike GEMM the hot-path contract names: out[M,N] = fmaf(A W^T, bn_a[n], bn_b[n])
 * with A (M,K) u8 spikes and W as planes (see above); a thin wrapper over sdf_spike_gemm_fwd. */
int sdf_spike_gemm_bn_fwd(const uint8_t* A_spike, const uint16_t* W_planes, int nsplit, float acc_scale, const float* bn_a,
                          const float* bn_b, float* out, int64_t M, int K, int N, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Window index table (row a4 / a6).  Replaces: F.pad to window multiples + torch.roll(-shift) + window_partition_v2 +
 * the raw `.view(Wd, B_, Wh, Ww, C)` (reference Spiking_swin_transformer3D.py:789-804, :100-113) and, read backwards,
 * window_reverse + roll(+shift) + crop (:810-820; swin_transformer3D_v2.py:52-65).
 * map[(j*Wh*Ww) + tok] = flat (b, d, h, w) index of token `tok` of slice j, or -1 for padding; slice j = window*Wd + frame,
 * windows ordered (b, d-block, h-block, w-block); attention step t' of window b' is slice t'*B_ + b'.  map holds
 * B_*Wd*Wh*Ww int32 (device memory of the caller); *n_windows (host, optional) receives B_.  Built by a kernel on `stream`. */
int sdf_window_slice_map(int32_t* map, int B, int D, int H, int W, int Wd, int Wh, int Ww, int shift_d, int shift_h, int shift_w,
                         int64_t* n_windows, void* stream);

/* Rows of a channel-last fp32 buffer moved through that table - the training path's window partition / reverse with no
 * materialised pad, roll, permute or crop:  gather  out[i,:] = map[i] >= 0 ? x[map[i],:] : 0   (M = map length rows out);
 * scatter  out[map[i],:] = y[i,:] for map[i] >= 0 (rows of `out` that no entry names are left untouched - every valid source
 * row occurs exactly once in a slice map, so each is the other's backward).  C % 4 == 0, 16-byte aligned. */
int sdf_rows_gather_fwd(const float* x, const int32_t* map, float* out, int64_t M, int C, void* stream);
int sdf_rows_scatter_fwd(const float* y, const int32_t* map, float* out, int64_t M, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spiking QK window attention, whole (rows a5 + a6):  x += SSA(x) in place.
 * Replaces: Spiking_SwinTransformerBlock3D.SSA + Spiking_QK_WindowAttention3D.forward + the shortcut add
 * (reference Spiking_swin_transformer3D.py:781-821, :661-717, :840).  TWO launches on `stream` where the first half has its
 * one-launch kernel (csrc/qk_front.hip: T' = 2, N1 <= 96, C % 96 == 0, fp16 planes, the four neurons of one class - the first
 * three steps below on a (slice pair, head) per workgroup, xs and q | k never in memory), else four:
 *   xs = SN_proj(x gathered through slice_map)                                  (T', B_*N1, C) u8
 *   q | k = SN_q/k( BN( xs [Wq;Wk]^T ) [+ positional_encoding on the k half] )  fused into the GEMM epilogue
 *   E = k AND SN2_q( sum over each head's 32 channels of q )                    (token gate)
 *   x[slice_map] += BN( Z Wp^T + b ),  Z = E read through the raw (B_,nH,T',N1,hd) head reshape (:709-710)
 * Weights are planes from sdf_split_weight_*; BN as (alpha, beta) per channel.  Give EITHER the stacked projection
 * (qk_*: planes [nsplit][2C][C], alpha / beta (2C), add (T', N1, 2C) with zeros in the q half, or NULL) - valid when the
 * q and k neurons are parameter-free and equal - OR the separate q_* / k_* sets (PSN: each neuron owns a matrix).
 * workspace: sdf_qk_attn_workspace_bytes(B_, T', N1, C) bytes, 256-byte aligned, caller-owned; gemm_workspace is the
 * optional split-K scratch of sdf_spike_gemm_fwd.  C = nH * 32. */
typedef struct SdfNeuronCfg {
  int32_t kind;             /* SDF_LIF | SDF_PSN | SDF_IF */
  float tau, v_th, v_reset;
  int32_t soft_reset;
  const float* psn_w;       /* (T,T), PSN only */
  const float* psn_b;       /* (T)          */
} SdfNeuronCfg;

typedef struct SdfQkAttnDesc {
  float* x;                 /* (B, D, H, W, C) fp32 channel-last, updated in place */
  const int32_t* slice_map; /* sdf_window_slice_map */
  int64_t B_;               /* windows */
  int64_t x_rows;           /* B*D*H*W */
  int32_t Tq, N1, C, nH;    /* window depth, Wh*Ww, channels, heads */
  int32_t nsplit;
  const uint16_t* qk_planes; const float* qk_alpha; const float* qk_beta; const float* qk_add; float qk_acc_scale;
  const uint16_t* q_planes;  const float* q_alpha;  const float* q_beta;  float q_acc_scale;
  const uint16_t* k_planes;  const float* k_alpha;  const float* k_beta;  const float* k_add; float k_acc_scale;
  const uint16_t* p_planes;  const float* p_bias;   const float* p_alpha; const float* p_beta; float p_acc_scale;
  SdfNeuronCfg sn_proj, sn_q, sn_k, sn2_q;
  void* workspace;      int64_t workspace_bytes;
  void* gemm_workspace; int64_t gemm_workspace_bytes;
  int32_t flags;        /* SDF_QK_* bits */
  /* Digit-plane stages (T' = 2, LIF / IF / PSN neurons, digit planes given - see below; round 5: csrc/ms_res.hip - whole-K weights LDS-resident, a
   * row loop per workgroup - for C in 64..768 in steps of 32 wherever K <= 1024, by default from 128 channels on; csrc/ms_wide.hip for C >= 192 in
   * steps of 64 beside it): with x_src set the call is THREE launches -
   * slice neuron, one kernel for q | k + BN + neurons + token gate, and the projection as a "position-major" product whose waves own
   * all xD time steps of a few positions of the (xB, xD, xHW, C) buffer x (xB * xD * xHW == x_rows):
   *   x_src   : int32 per row of x, made by sdf_window_zsrc_map from slice_map (where that row's gated spikes start in E); NULL = the
   *             general kernels above
   *   emit_s1 : optional u8 [x_rows][C]: receives SN_emit( x after the update ) over the xD steps of every position - the first
   *             neuron of the MLP that follows (reference Spiking_swin_transformer3D.py:168; hand it to SdfMsMlpDesc.s1_in), so the
   *             updated x is not read again; emit_sn = that neuron (LIF / IF / PSN with its T = xD matrix).  Layout: the TILED hand-over form
   *             ([80-row unit][C / 16][row][16 B], (x_rows + 80) * C bytes) - opaque to the caller - unless SDF_QK_KEEP_SPIKES is
   *             set: then plain row-major [x_rows][C] (the parity tape). */
  const int32_t* x_src;
  int32_t xB, xD;
  int64_t xHW;
  uint8_t* emit_s1;
  SdfNeuronCfg emit_sn;
  /* The wide-stage kernels multiply on the int8 matrix pipe (spike bytes are int8 values): the same weights again as digit planes
   * int8_t[3][rows][C] + one power-of-two scale per output channel, made by sdf_split_weight_i8x3 (stacked [Wq; Wk] as 2C rows for
   * the qk_* form, else q_* and k_*; p_* = the output projection).  All NULL = the general kernels on the 16-bit planes above. */
  const int8_t* qk_digits; const float* qk_cscale;
  const int8_t* q_digits;  const float* q_cscale;
  const int8_t* k_digits;  const float* k_cscale;
  const int8_t* p_digits;  const float* p_cscale;
  /* Round 6 - several independent batch-1 forwards in one call ("replicas"): the B_ windows are B_ / rep_windows problems of
   * rep_windows windows each.  slice_map (and x_src) are the caller's concatenation of the per-replica tables - entry
   * (t' * B_ + r * rep_windows + b') * N1 + n = r * x_rows_1 + map_1[(t' * rep_windows + b') * N1 + n] - so steps 1 - 3 run unchanged on
   * the (T', B_, N1, C) workspace; only the head scramble of step 4 is per replica (SdfSpikeGemmDesc.zg_rep).  0 = one problem (the
   * reference's own batch semantics, which couples the samples of a batch through window_partition_v2's raw view).  rep_windows % T' == 0. */
  int32_t rep_windows;
} SdfQkAttnDesc;

enum {
  SDF_QK_KEEP_SPIKES = 1,    /* leave the q | k spikes in `workspace` behind E (what the four-launch form always does; the parity tape) */
  SDF_QK_FOUR_LAUNCHES = 2,  /* never take the one-launch first half (A/B reference; same as SDF_QK_FRONT=0 in the environment) */
  SDF_QK_NARROW = 4          /* never take the wide-stage kernels (A/B reference; same as SDF_WIDE=0 in the environment) */
};

/* Inverse of the slice map for the projection's head scramble (reference Spiking_swin_transformer3D.py:709-710): x_src[r] = byte offset
 * in the gated-spike tensor E (T', B_, N1, C) of Z[t, b, n, 0] for the slice-map entry (t, b, n) that names row r of x; rows no entry
 * names keep their old value (there are none for a map made by sdf_window_slice_map over the same x).  x_src: int32 [x_rows]. */
int sdf_window_zsrc_map(const int32_t* slice_map, int64_t B_, int Tq, int N1, int nH, int32_t* x_src, void* stream);

int64_t sdf_qk_attn_workspace_bytes(int64_t B_, int Tq, int N1, int C);
int sdf_qk_attn_fwd(const SdfQkAttnDesc* d, void* stream);
/* 1 when sdf_qk_attn_fwd will run this descriptor on the wide-stage kernels (and therefore honours emit_s1), else 0; host-only. */
int sdf_qk_attn_is_wide(const SdfQkAttnDesc* d);

/* ---------------------------------------------------------------------------------------------
 * MS MLP, whole (row a7):  x += BN2( SN2( BN1( SN1(x) W1^T ) ) W2^T )  in place on a (B, D, HW, C) fp32 buffer, neurons over
 * the true time axis D.  Replaces: MS_Spiking_Mlp.forward + the block's second shortcut add (reference
 * Spiking_swin_transformer3D.py:164-181, :845).  ONE launch (csrc/ms_mlp_fused.hip: SN1, fc1, BN1, SN2, fc2, BN2 and the
 * shortcut on a tile of positions x all D steps; neither spike tensor leaves the compute unit) for C in {96, 192},
 * D in {5,10,20}, Ch % 96 == 0; otherwise three launches with the hidden (.., 4C) tensor as 1-byte spikes in `workspace`
 * (D in {2,4,5,10,20}, the fused-neuron GEMM epilogue).  workspace: sdf_ms_mlp_workspace_bytes(B*D*HW, C, Ch), 256-byte aligned. */
typedef struct SdfMsMlpDesc {
  float* x;
  int32_t B, D;
  int64_t HW;
  int32_t C, Ch, nsplit;
  const uint16_t* fc1_planes; const float* fc1_alpha; const float* fc1_beta; float fc1_acc_scale;
  const uint16_t* fc2_planes; const float* fc2_alpha; const float* fc2_beta; float fc2_acc_scale;
  SdfNeuronCfg sn1, sn2;
  void* workspace;      int64_t workspace_bytes;
  void* gemm_workspace; int64_t gemm_workspace_bytes;
  int32_t flags;        /* SDF_MLP_* bits */
  /* Digit-plane stages (C >= 64 in steps of 32 up to 192 and Ch <= 768 - csrc/ms_res.hip - or C >= 192 in steps of 64; LIF / IF / PSN, digit planes
   * given - see below, D in {10, 20}; by default taken from 128 channels on): fc1 + BN1 + SN2 and fc2 + BN2 + shortcut as two
   * position-major launches.  s1_in != NULL: the SN1 spikes are already at the head of `workspace` (written there by
   * SdfQkAttnDesc.emit_s1 == workspace; tiled, or row-major when both calls carry their KEEP_SPIKES flag): no neuron launch, x is
   * only read by the last launch's shortcut.  Without SDF_MLP_KEEP_SPIKES the hidden spikes travel in the tiled form too. */
  const uint8_t* s1_in;
  /* the weights again as int8 digit planes int8_t[3][N][K] + a power-of-two scale per output channel (sdf_split_weight_i8x3): what
   * the wide-stage kernels multiply by; NULL = the general kernels on the 16-bit planes above. */
  const int8_t* fc1_digits; const float* fc1_cscale;
  const int8_t* fc2_digits; const float* fc2_cscale;
  /* wide-stage form only: emit_next != NULL (u8 [tokens][C], row-major) also receives SN_emit( x after the update ) over the D steps of
   * every position - the first neuron of whatever reads x next (the patch merging's `sn`, reference Spiking_swin_transformer3D.py:970,
   * or MS_ResBlock.sn1 of the U-Net bottleneck, Spiking_modules.py:922) - from the last launch's epilogue, so x is not read again. */
  uint8_t* emit_next;
  SdfNeuronCfg emit_sn;
  /* wide-stage form, optional: fc2's digits again in MFMA fragment order (sdf_tile_weight_i8x3 of fc2_digits; fc2_cscale serves both).
   * With it fc2 runs on the small-M kernel (csrc/ms_smallm.hip: K split over the waves of a workgroup, two workgroups per compute
   * unit) instead of the wide main loop where its (80-row unit x 32-column) tiles fit the chip in one round (<= 512 tiles: swin stage 3 at
   * batch 1, 30.9 -> 19.9 us) - bit-equal results; NULL = the wide main loop. */
  const int8_t* fc2_tiled;
} SdfMsMlpDesc;

enum {
  SDF_MLP_KEEP_SPIKES = 1,   /* leave SN1's and SN2's spikes in `workspace` (u8 [tokens][C], then [tokens][Ch] at the next 256-byte
                                boundary): what the three-launch form always does; the one-launch form only on request */
  SDF_MLP_THREE_LAUNCHES = 2,/* never take the one-launch kernel (A/B reference; same as SDF_MLP_FUSED=0 in the environment) */
  SDF_MLP_NARROW = 4         /* never take the wide-stage kernels (A/B reference; same as SDF_WIDE=0 in the environment) */
};

int64_t sdf_ms_mlp_workspace_bytes(int64_t tokens, int C, int Ch);
int sdf_ms_mlp_fwd(const SdfMsMlpDesc* d, void* stream);
/* 1 when sdf_ms_mlp_fwd will run this descriptor on the wide-stage kernels (and therefore accepts s1_in), else 0; host-only. */
int sdf_ms_mlp_is_wide(const SdfMsMlpDesc* d);

/* ---------------------------------------------------------------------------------------------
 * MS patch merging on spikes (row a8):  out = BN( cat_2x2( S ) W^T ),  S = SN(x) as u8 (B, D, H, W, C), W (N, 4C) given as int8 digit
 * planes, out (B, D, ceil(H/2), ceil(W/2), N) fp32 (odd sizes read zero spikes, the reference's F.pad in front of the neuron).  Replaces MS_SpikingPatchMerging.forward behind its neuron (reference
 * Spiking_swin_transformer3D.py:965-972: the four strided slices, the concatenation along channels in quadrant order
 * (dh, dw) = (q % 2, q / 2), sj_layer.Linear, the BatchNorm) - the concatenation is index arithmetic in the operand loads of the
 * digit main loops (csrc/ms_res.hip for C <= 256 in steps of 32: any row count; csrc/ms_wide.hip for C % 64 == 0: at most 32 000 output
 * rows), nothing is materialised.  N % 32 == 0, D in {10, 20}; SDF_E_SHAPE otherwise (the caller keeps its gather map + sdf_spike_gemm_fwd). */
typedef struct SdfMsMergeDesc {
  const uint8_t* spikes;
  const int8_t* digits; const float* cscale;   /* sdf_split_weight_i8x3 of the (N, 4C) reduction weight */
  const float* alpha; const float* beta;       /* BatchNorm as (alpha, beta) per output channel, or NULL */
  float* out;
  int32_t B, D, H, W, C, N;
} SdfMsMergeDesc;

int sdf_ms_patch_merge_fwd(const SdfMsMergeDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Stride-2 3x3 transposed convolution on spikes as ONE product (round 5; csrc/ms_res.hip):
 *   out[img, oy, ox, co] = alpha[co] * sum_{ky, kx, c : oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx} S[img, iy, ix, c] W[c, co, ky, kx] + beta[co]
 * - `layer.ConvTranspose2d(3, stride 2, padding 1, output_padding 1)` + the decoder's BatchNorm behind its neuron (reference
 * MS_SpikingTransposeDecoderLayer, Spiking_modules.py:461-474).  A row of the product is an input pixel (img, a, b), its K = 4 Cin the
 * 2 x 2 input neighbourhood (a..a+1, b..b+1; zero beyond the image) in patch merging's quadrant order (dh, dw) = (q % 2, q / 2), its
 * N = 4 Cout columns the four output pixels (2a + py, 2b + px) of the row's 2 x 2 output block, column (2 py + px) Cout + co: the weight
 * matrix holds W[., ., ky, kx] in the blocks a tap reaches and zeros elsewhere (7 of 16 blocks), as int8 digit planes
 * (sdf_split_weight_i8x3 of the (4 Cout, 4 Cin) matrix).  The four parity-class convolutions it replaces wrote every other pixel of a
 * row each (half-written 128-byte lines: twice the output's bytes reached HBM); here a row's two output pixels of a line are stored together.
 * S (imgs, H, W, Cin) u8 NHWC, imgs % T == 0 with T in {10, 20}; Cin % 16 == 0, 4 Cin <= 1024; Cout % 8 == 0; out (imgs, 2H, 2W, Cout)
 * fp32; alpha / beta (4 Cout): the BatchNorm pair of channel co at every column (2 py + px) Cout + co, or NULL.  SDF_E_SHAPE otherwise
 * (the caller keeps sdf_spike_conv2d_multi_fwd). */
typedef struct SdfSpikeDeconvDesc {
  const uint8_t* spikes;
  const int8_t* digits; const float* cscale;   /* [3][4 Cout][4 Cin] + (4 Cout) */
  const float* alpha; const float* beta;       /* (4 Cout) or NULL */
  float* out;
  int32_t imgs, T, H, W, Cin, Cout;
} SdfSpikeDeconvDesc;

int sdf_spike_deconv3x3s2_fwd(const SdfSpikeDeconvDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spike convolution (implicit GEMM):  out = epilogue( im2col(X) x W^T ) with X an NHWC u8 spike image batch.
 * Replaces: layer.Conv2d / nn.Conv2d / ConvTranspose2d on spikes + the SpikingNormLayer, shortcut add and
 * Spiking_neuron around it in the patch embedding and the U-Net tail (reference Spiking_modules.py:339-347,
 * 467-474, 811-818, 906-926).  `g` is used as in sdf_spike_gemm_fwd with:
 *   g.A  = X (imgs, H, W, Cin) u8, Cin % 16 == 0, Cin >= 48;   g.M = imgs*OH*OW;   g.N = Cout (multiple of 96)
 *   g.K  = KH*KW*Cin, weights packed [nsplit][Cout][(ky, kx, cin)] bf16 planes
 *   row m = (img, oy, ox) reads input pixel (oy*sy + dy[ky], ox*sx + dx[kx]); zero outside the image
 *     (a 3x3 / pad 1 convolution: dy = dx = {-1, 0, 1}; the parity classes of a stride-2 transposed convolution
 *     are 1- or 2-tap grids with their own offsets and an out_rowmap that places the class's outputs)
 *   epilogue: the fp32 one (alpha/beta/resid/out_rowmap, out is (rows, Cout) fp32 NHWC) or, with sn_T == 10 (int8 digit
 *     planes on the weight-resident kernel: also 5 and 20, its time loop is rolled),
 *     the fused neuron (out_spike u8 NHWC); pos_* describe how the imgs dimension factors into (time, position).
 *     With sn_T > 0 and g.out != NULL the pre-activation  fmaf(acc, alpha, beta) (+ g.resid)  is ALSO stored to g.out
 *     (fp32, row stride g.ldo) and the neuron runs on that sum: MS_ResBlock's conv2 -> BN -> + identity and the next
 *     block's sn1 in one launch (reference Spiking_modules.py:922-933).
 */
typedef struct SdfSpikeConvDesc {
  SdfSpikeGemmDesc g;
  int32_t H, W, Cin, OH, OW;
  int32_t KH, KW, sy, sx;
  int32_t dy[3], dx[3];
} SdfSpikeConvDesc;

int sdf_spike_conv2d_fwd(const SdfSpikeConvDesc* c, void* stream);
/* n (1 .. 4 fused) convolutions with the fp32 epilogue on the SAME images and output buffer that differ only in taps (KH, KW, dy, dx),
 * weights and g.out_rowmap - the four output-parity classes of ConvTranspose2d(k 3, s 2, p 1, op 1) in MS_SpikingTransposeDecoderLayer
 * (reference Spiking_modules.py:461-474), whose row maps write disjoint rows: ONE launch where the library's streaming kernel serves
 * every one of them (each class alone fills about half of the chip), otherwise exactly n calls of sdf_spike_conv2d_fwd in order. */
int sdf_spike_conv2d_multi_fwd(const SdfSpikeConvDesc* cs, int n, void* stream);

/* W (fp32, n elements) -> nsplit bf16 planes (round-to-nearest-even residual split). */
int sdf_split_weight_bf16(const float* W, uint16_t* planes, int64_t n, int nsplit, void* stream);

/* W (fp32, n elements) -> two fp16 planes [2][n] with  scale * W = hi + lo  (|error| <= 2^-22 |W|).  `scale` is a
 * power of two chosen by the caller so that scale * max|W| < 2^15 (fp16 range; small weights stay far above the
 * fp16 subnormal spacing); pass acc_scale = 1 / scale with nsplit = 2.  Spikes are exact in fp16, the MFMA
 * accumulates in fp32 and the rescaling is exact, so the result differs from the 3-plane one only by the 2^-22
 * weight truncation - below the rounding noise of the fp32 accumulation itself - at 2/3 of its MFMA work. */
int sdf_split_weight_f16x2(const float* W, uint16_t* planes, int64_t n, float scale, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token gate of Spiking_QK_WindowAttention3D (reference Spiking_swin_transformer3D.py:687-694):
 *   a[t,b,n,g] = sum_{d<32} q[t,b,n,g*32+d] ; A = neuron_T'(a) ; E = k * A (broadcast over d).
 * q, k, e: u8 spikes laid out (Tq, rows, C) with rows = B_*N1, C % 32 == 0; the neuron runs over Tq
 * with the same kind/params semantics as sdf_neuron_fwd (LIF | PSN).
 */
int sdf_qk_gate_fwd(const uint8_t* q, const uint8_t* k, uint8_t* e, int Tq, int64_t rows, int C,
                    int kind, float tau, float v_th, float v_reset, int soft_reset,
                    const float* psn_w, const float* psn_b, void* stream);
/* Same, with q and k rows ldq / ldk bytes apart (multiples of 16, >= C): q and k may be the two halves of the
 * (Tq*rows, 2C) output of ONE fused-neuron spike GEMM over the stacked weights [Wq; Wk].  e stays (Tq, rows, C). */
int sdf_qk_gate_strided_fwd(const uint8_t* q, const uint8_t* k, uint8_t* e, int Tq, int64_t rows, int C,
                            int64_t ldq, int64_t ldk, int kind, float tau, float v_th, float v_reset,
                            int soft_reset, const float* psn_w, const float* psn_b, void* stream);
/* The strided gate with a GLIF gate node: A = GLIF_T'(a) from v = 0, s = 0 with `tab` = [L, Dk, g, R, th, c_0 .. c_{Tq-1}] in DEVICE
 * memory; Tq in {2, 4}.  `gate` (Tq, rows, C / 32) u8, when not NULL, also receives A itself.  C, ldq, ldk and alignment as above. */
int sdf_qk_gate_glif_fwd(const uint8_t* q, const uint8_t* k, uint8_t* e, uint8_t* gate, const float* tab, int Tq, int64_t rows,
                         int C, int64_t ldq, int64_t ldk, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Head of the patch embedding: conv3x3 / pad 1 (no bias) on the real-valued event voxel -> eval BatchNorm -> neuron over T,
 * one kernel, spikes out.  Replaces MS_PED_Spiking_PatchEmbed_Conv_sfn.head (reference Spiking_modules.py:1782).
 *   x   (B*T, H, W, Cin) fp32, NHWC, image index = b*T + t          w (Cout, Cin, 3, 3) fp32 (the module's layout)
 *   out (B*T, H, W, Cout) u8 spikes                                  alpha / beta (Cout) or NULL
 * Accumulation: fp32 products and sums in (ky, kx, cin) order - on the exact fp32 matrix pipe (v_mfma_f32_32x32x2_f32) when
 * W % 32 == 0 (LIF / IF; the PSN for T <= 10 and Cin = 2: its H is accumulated on the fly per 32-channel block), else one fmaf
 * chain per output on the vector pipe.  Built for (Cin, Cout) in {(2,32), (2,48), (2,64), (4,48)}, T in {5, 10, 20}, W % 16 == 0; anything else returns
 * SDF_E_SHAPE and the caller keeps its library convolution + sdf_neuron_fwd pair.
 */
typedef struct SdfHeadConvDesc {
  const float* x;
  const float* w;
  const float* alpha;
  const float* beta;
  uint8_t* out;
  int32_t B, T, H, W, Cin, Cout;
  int32_t sn_kind;
  float tau, v_th, v_reset;
  int32_t soft_reset;
  const float* psn_w;
  const float* psn_b;
  /* strided input (all zero = the packed NHWC layout above): element (b, t, y, x, ci) of the input is
   * x[b * x_sb + t * x_st + y * x_sy + x * x_sx + x_sc[ci]] - the event voxel (B, bins, 2, H, W) is then read IN PLACE
   * (reference patch embedding :1775-1784: time step t takes bin t of each polarity; channel ci = (bin group, polarity)),
   * no re-layout copies in front of the kernel */
  int64_t x_sb, x_st, x_sy, x_sx;
  int64_t x_sc[4];
} SdfHeadConvDesc;

int sdf_head_conv_sn_fwd(const SdfHeadConvDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * 1x1 strided convolution of a real-valued fp32 NHWC image on the exact fp32 matrix pipe (csrc/pointwise_conv.hip):
 *   out[img, oy, ox, n] = sum_c x[img, oy*stride, ox*stride, c] * w[n, c] (+ bias[n])
 * Replaces SpikingPEDLayer.conv_res - the membrane shortcut of the stride-2 patch-embedding projection, the one layer of the
 * SNN forward that reads a membrane instead of spikes (reference Spiking_modules.py:772-826).
 *   x (imgs, H, W, Cin) fp32; w (N, Cin) fp32 (the module's (N, Cin, 1, 1)); out (imgs, OH, OW, N) fp32, OH = (H-1)/stride + 1.
 * Built for Cin = 96, N in {96, 192}; anything else returns SDF_E_SHAPE and the caller keeps its library convolution. */
typedef struct SdfPointwiseConvDesc {
  const float* x;
  const float* w;
  const float* bias;        /* (N) or NULL */
  float* out;
  int32_t imgs, H, W, Cin, N, stride, OH, OW;
} SdfPointwiseConvDesc;

int sdf_pointwise_conv_f32_fwd(const SdfPointwiseConvDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * col2im + eval BatchNorm of a ConvTranspose2d(k=3, s=2, p=1, output_padding=1) on spikes whose nine per-tap products were
 * computed by ONE plain sdf_spike_gemm_fwd over the stacked tap weights (N = 9*Cout, column = (ky*3+kx)*Cout + co):
 *   out[img, oy, ox, co] = fmaf( sum_{taps reaching (oy,ox)} Y[(img, iy, ix)][(ky*3+kx)*Cout + co], alpha[co], beta[co] ),
 *   oy = 2*iy - 1 + ky, ox = 2*ix - 1 + kx.   Replaces MS_SpikingTransposeDecoderLayer's deconv + norm
 * (reference Spiking_modules.py:461-474) for the small decoder levels, where one GEMM fills the chip and four
 * parity-class convolutions (the other form this library offers, see sdf_spike_conv2d_fwd) do not.
 *   Y (imgs*H*W, 9*Cout) fp32;  out (imgs, 2H, 2W, Cout) fp32;  alpha / beta (Cout) or NULL;  Cout % 4 == 0.
 */
int sdf_deconv_col2im_fwd(const float* Y, const float* alpha, const float* beta, float* out, int imgs, int H, int W,
                          int Cout, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Flow read-out: out[b,c,Y,X] = sum_t pred[b,t,ys,xs,c] with (ys, xs) the nearest-neighbour source pixel of (Y, X) for
 * scale factors (scale_y, scale_x) - exactly F.interpolate(pred.sum(time), scale_factor=...)
 * (reference Spiking_STSwinNet.py:289-303).  pred is (B, D, h, w, ldp) fp32 of which the first C columns are read;
 * out is (B, C, H, W) fp32.
 */
int sdf_flow_out_fwd(const float* pred, float* out, int B, int D, int h, int w, int64_t ldp, int C, int H, int W,
                     float scale_y, float scale_x, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Flow-prediction head of one U-Net level, one launch (csrc/pred_head.hip):
 *   p[t] = conv1x1(SN_pred(z)[t]) + bias (2 outputs; MS_SpikingPredLayer, reference Spiking_modules.py:605-640),
 *   flow = nearest upsampling by whole factors (H / h, W / w) of sum_t p[t] (reference Spiking_STSwinNet.py:289-303), and - the
 *   next decoder level reads cat(p, z, skip) behind its own neuron (Spiking_STSwinNet.py:168-172, Spiking_modules.py:467-474) -
 *   the spike bytes of SN_next(z) / SN_next(p) written into their channel slices of that level's NHWC u8 spike image.
 * Replaces sdf_neuron_fwd + sdf_spike_gemm_fwd (2 columns padded to 32) + sdf_flow_out_fwd of this level and two
 * sdf_neuron_fwd launches (+ the zero fill of the image's padding channels) of the next one; z is read once.
 *   z (B, D, h*w, Cin) fp32 channel-last; Cin in {96, 192, 384}; D in {5, 10, 20} (PSN: D <= 10); wgt (2, Cin) fp32; bias (2) or NULL
 *   pred (B, D, h*w, 4) fp32 = (p0, p1, 0, 0) or NULL;  flow (B, 2, H, W) fp32 or NULL (H % h == 0, W % w == 0)
 *   next_spikes (B, D, h*w, next_ld) u8 or NULL: bytes [next_z_off, +Cin) = SN_next(z), [next_pred_off, +4) = SN_next(p) (channels
 *     2, 3 zero), [next_zero_off, +next_zero_len) zeroed (the image's padding channels); all offsets / lengths multiples of 4
 *   keep_spikes (B, D, h*w, Cin) u8 or NULL: SN_pred(z) (parity tape).  Anything else returns SDF_E_SHAPE: the caller keeps the
 *   three-launch form. */
typedef struct SdfPredHeadDesc {
  const float* z;
  int32_t B, D, h, w, Cin;
  SdfNeuronCfg sn_pred;
  const float* wgt;                 /* (2, Cin) fp32 */
  const float* bias;
  float* pred;
  float* flow;
  int32_t H, W;
  uint8_t* next_spikes;
  int32_t next_ld, next_z_off, next_pred_off, next_zero_off, next_zero_len;
  SdfNeuronCfg sn_next;
  uint8_t* keep_spikes;
} SdfPredHeadDesc;

int sdf_pred_head_fwd(const SdfPredHeadDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Eval BatchNorm affine (+ residual):  out = fmaf(x, alpha[c], beta[c]) (+ resid), c = (i/inner) % C.
 * Replaces: SpikingNormLayer after a convolution and the membrane (MS) shortcut add
 * (reference Spiking_modules.py:922-926, 816-818).  n % 4 == 0; inner % 4 == 0 or (inner == 1, C % 4 == 0).
 * `resid` may be NULL; `out` may alias `x` or `resid`.
 */
int sdf_affine_resid_fwd(const float* x, const float* alpha, const float* beta, const float* resid, float* out,
                         int64_t n, int C, int64_t inner, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused 3-D window attention over (window, head): scores + relative-position bias (+ shift mask)
 * [+ softmax] times V, head_dim 32, up to 192 tokens per window.
 *   SDF_ATTN_ANN replaces WindowAttention3D.forward's core (reference
 *     models/STSwinNet/swin_transformer3D_v2.py:176-202): `q` points at the packed qkv projection output
 *     (B_, N, 3, nH, 32) fp32 (k, v are ignored but must be non-NULL); cosine attention
 *     normalize(q) normalize(k)^T * scale[g] + bias[g] (+ mask[b % nW]) -> softmax -> @ v;
 *     out (B_, N, nH*32) fp32.  scale[g] = exp(min(logit_scale[g], ln 100)); bias = 16*sigmoid(cpb(...)).
 *   SDF_ATTN_SEW replaces Spiking_BN_WindowAttention3D.forward's core (reference
 *     models/STSwinNet_SNN/Spiking_swin_transformer3D.py:320-363): q, k, v are u8 spikes in the reference's
 *     raw head view (B_, nH, N, 32) of the (T', B_, N1, C) buffers; (q*scale[g]) k^T + bias[g] (+ mask), NO
 *     softmax, @ v; out fp32 (T', B_, N1, C) through the (B_,nH,T',N1,hd) -> (T',B_,N1,C) scramble.
 * bias is (nH, N, N) fp32, mask (nW, N, N) fp32 or NULL.  All matrix products run on the exact fp32 MFMA.
 * More than 192 tokens per window: sdf_win_attn_large_fwd.
 */
enum { SDF_ATTN_ANN = 0, SDF_ATTN_SEW = 1 };
typedef struct SdfWinAttnDesc {
  int32_t mode;
  const void* q;
  const void* k;
  const void* v;
  float* out;
  int32_t B_, nW, nH, N, hd;
  int32_t Tq, N1;           /* SEW only: N == Tq*N1 */
  const float* scale;       /* (nH) */
  const float* bias;        /* (nH,N,N) */
  const float* mask;        /* (nW,N,N) or NULL */
  /* ANN mode, optional in-kernel windowing (replaces F.pad + torch.roll + window_partition in front of the attention and
   * window_reverse + roll back + crop behind it, reference swin_transformer3D_v2.py:286-310): row_map[b_*N + n] = row of
   * token n of window b_ in the un-partitioned (rows, 3C) qkv buffer and (rows, C) output buffer (the table of
   * sdf_window_slice_map), or -1 for a padding token; a padding token's q | k | v is pad_qkv (3C floats: what the qkv
   * Linear makes of a zero row, i.e. its bias) and its output row is dropped.  NULL = q and out are window-major. */
  const int32_t* row_map;
  const float* pad_qkv;
} SdfWinAttnDesc;

int sdf_win_attn_fwd(const SdfWinAttnDesc* d, void* stream);

/* ---- the same attention for larger windows: 192 < N <= 1024 tokens (up to window (2,22,22)) ------------------------------------
 * Descriptor, modes, layouts and arithmetic of sdf_win_attn_fwd (exact fp32 MFMA for both products, the score rounded as
 * (acc * scale + bias) + mask), with the keys walked in blocks of 64: the ANN mode keeps a running row maximum and sum (online
 * softmax), the SEW mode only accumulates.  Argument checks are those of sdf_win_attn_fwd in the same order, except the range:
 * N <= 192 or N > 1024 is SDF_E_SHAPE.  Everything is refused before any launch; one launch; no atomics, two calls give bit-equal
 * results.  Its backward: sdf_win_attn_large_ann_bwd / sdf_win_attn_large_sew_bwd below (the first two backward entry points serve
 * N <= 192). */
int sdf_win_attn_large_fwd(const SdfWinAttnDesc* d, void* stream);

/* ---- the attention map of the same attention: 1 <= N <= 1024 tokens (`return_attention=True`, `log=True`) --------------------------
 * What the reference's attention modules return as their second value, scores (B_, nH, N, N) fp32, window-major:
 * scores[((b * nH + g) * N + i) * N + j].  Descriptor, modes, operand layouts and arithmetic of sdf_win_attn_fwd (exact fp32 MFMA,
 * the score rounded as (acc * scale + bias) + mask); d->v and d->out are ignored and may be NULL.
 *   SDF_ATTN_ANN: softmax over the keys of normalize(q) normalize(k)^T * scale[g] + bias[g] (+ mask[b % nW]) (reference
 *     swin_transformer3D_v2.py:176-202), through row_map / pad_qkv as sdf_win_attn_fwd reads them: a padding token is a row and a
 *     column of the map.  The keys are walked twice (row maximum and sum, then exp(s - max) / sum); no workspace.
 *   SDF_ATTN_SEW: (q * scale[g]) k^T + bias[g] (+ mask), no softmax (Spiking_swin_transformer3D.py:320-360): the accumulator is the
 *     exact count c of common spikes and the element is fp32(fp32(c * scale[g]) + bias) (+ mask).
 * One kernel for every N, keys in blocks of 64, one launch; no atomics, two calls give bit-equal results.  Checks, before any
 * launch, in sdf_win_attn_fwd's order: NULL d, q, k (SEW), scale, bias, row_map without pad_qkv -> SDF_E_NULL; unknown mode ->
 * SDF_E_DTYPE; hd != 32, B_ / nH / N < 1, N > 1024, SEW Tq * N1 != N, a mask with nW < 1 or B_ % nW != 0, SEW with a row_map ->
 * SDF_E_SHAPE; then scores NULL -> SDF_E_NULL, scores not 4-byte aligned (or q / k / pad_qkv not aligned as sdf_win_attn_fwd
 * needs them) -> SDF_E_ALIGN.  Added to SDF_VERSION 107 (no existing entry changed). */
int sdf_win_attn_scores_fwd(const SdfWinAttnDesc* d, float* scores, void* stream);

/* ---- backward of the SDF_ATTN_ANN core of sdf_win_attn_fwd (training of the ANN model) -------------------------------------
 * Per window b and head g: q^ = q / max(|q|, 1e-12), k^ likewise, S = q^ k^T * scale[g] + bias[g] (+ mask[b % nW]),
 * P = softmax(S), O = P v.  Given dout = dL/dO (rows, C) through the same row map (D = rowsum(dO o O) is formed as
 * rowsum(P o dP) from the recomputed P, so the forward's output is not an input):
 *   dqkv (rows, 3C): dL/d(q | k | v) of every real row (written through row_map; each real row lies in exactly one window);
 *   d_pad (3C): the summed dq | dk | dv of all padding tokens (they read pad_qkv: part of the qkv bias gradient);
 *   d_scale (nH) = sum dS o (q^ k^T);  d_bias (nH, N, N) = sum over windows of dS.
 * qkv, row_map, pad_qkv, scale, bias, mask as in SdfWinAttnDesc (ANN mode; row_map NULL = window-major rows, d_pad may then be
 * NULL).  head_dim 32, N <= 192, any nH; SDF_E_SHAPE otherwise.  Exact fp32 MFMA products.  The cross-window sums go through
 * `workspace` (sdf_win_attn_ann_bwd_workspace_bytes(B_, nH, N) bytes, 256-byte aligned, caller-owned) in a fixed order: two
 * calls give bit-equal results. */
typedef struct SdfWinAttnBwdDesc {
  const float* qkv;         /* (rows, 3C) */
  const int32_t* row_map;   /* (B_*N) or NULL */
  const float* pad_qkv;     /* (3C), required with row_map */
  const float* dout;        /* (rows, C) */
  const float* scale;       /* (nH) */
  const float* bias;        /* (nH,N,N) */
  const float* mask;        /* (nW,N,N) or NULL */
  float* dqkv;              /* (rows, 3C) */
  float* d_pad;             /* (3C), required with row_map */
  float* d_scale;           /* (nH) */
  float* d_bias;            /* (nH,N,N) */
  void* workspace;
  int64_t workspace_bytes;
  int32_t B_, nW, nH, N, hd;
} SdfWinAttnBwdDesc;

int64_t sdf_win_attn_ann_bwd_workspace_bytes(int B_, int nH, int N);   /* 0 for an unsupported shape */
int sdf_win_attn_ann_bwd(const SdfWinAttnBwdDesc* d, void* stream);

/* ---- backward of the SDF_ATTN_SEW core of sdf_win_attn_fwd (training of the SEW model family) ------------------------------
 * Per window b and head g: A = scale[g] Q K^T + bias[g] (+ mask[b % nW]), O = A V, no softmax; Q, K, V the raw head view
 * (B_, nH, N, 32) of the (T', B_, N1, C) u8 spike buffers, O leaving through the (B_,nH,T',N1,hd) -> (T',B_,N1,C) scramble.
 * Given dout = dL/dO in that scrambled (T', B_, N1, C) layout:
 *   dq = scale dO (V^T K),  dk = scale V (dO^T Q),  dv = scale K (Q^T dO) + (bias[g] + mask)^T dO   (fp32, raw head view of q / k / v);
 *   d_bias (nH, N, N) = sum over windows of dO V^T.  The mask gets no gradient.
 * head_dim 32, N = Tq * N1 <= 192, any nH; SDF_E_SHAPE otherwise.  fp32 FMA on the vector ALU (spikes exact, dO and the 32 x 32
 * Gram matrices fp32).  d_bias goes through fixed-order split-K partials in `workspace`
 * (sdf_win_attn_sew_bwd_workspace_bytes(B_, nH, N) bytes, 256-byte aligned, caller-owned): no atomics, two calls give bit-equal
 * results. */
typedef struct SdfWinAttnSewBwdDesc {
  const uint8_t* q;         /* (T', B_, N1, C) spikes */
  const uint8_t* k;
  const uint8_t* v;
  const float* dout;        /* (T', B_, N1, C) */
  const float* scale;       /* (nH) */
  const float* bias;        /* (nH,N,N) */
  const float* mask;        /* (nW,N,N) or NULL */
  float* dq;                /* (T', B_, N1, C) each */
  float* dk;
  float* dv;
  float* d_bias;            /* (nH,N,N) */
  void* workspace;
  int64_t workspace_bytes;
  int32_t B_, nW, nH, Tq, N1, hd;
} SdfWinAttnSewBwdDesc;

int64_t sdf_win_attn_sew_bwd_workspace_bytes(int B_, int nH, int N);   /* 0 for an unsupported shape */
int sdf_win_attn_sew_bwd(const SdfWinAttnSewBwdDesc* d, void* stream);

/* ---- the two backward passes for larger windows: 192 < N <= 1024 tokens (the backward of sdf_win_attn_large_fwd) ---------------------
 * Descriptors, layouts and arithmetic of sdf_win_attn_ann_bwd / sdf_win_attn_sew_bwd, with keys and queries walked in blocks of 64
 * tokens: neither LDS nor registers depend on N.  Argument checks are those of the first two in the same order, except the range:
 * N <= 192 or N > 1024 is SDF_E_SHAPE (workspace queries: 0).  Everything is refused before any launch.
 *   ANN: a flash-style backward - a query-major kernel walks the keys twice (online softmax -> row maximum, 1 / row sum and
 *     D = rowsum(P o dP) per query, kept in the workspace; then dS, dq^ and the d_scale term), a key-major kernel walks the queries
 *     (dv, dk^), and d_bias is split-K over fixed runs of windows that recompute dS from the stored row statistics.  Exact fp32 MFMA
 *     products, the score rounded as (acc * scale + bias) + mask, a key past N contributes nothing; bias and mask must be finite.
 *   SEW: the Gram form of sdf_win_attn_sew_bwd with the Grams, dq / dk and the (bias + mask)^T dO walk streaming 64-token blocks, and
 *     the d_bias kernel staging V per 256-key block.
 * The workspace holds per-query row statistics, per-workgroup d_pad / d_scale partials and the d_bias run partials (a number of
 * runs bounded by the shape of one window, not by B_): no buffer grows as B_ * nH * N^2.  No atomics; d_pad, d_scale and d_bias are
 * summed in a fixed order: two calls give bit-equal results. */
int64_t sdf_win_attn_large_ann_bwd_workspace_bytes(int B_, int nH, int N);   /* 0 for an unsupported shape */
int sdf_win_attn_large_ann_bwd(const SdfWinAttnBwdDesc* d, void* stream);
int64_t sdf_win_attn_large_sew_bwd_workspace_bytes(int B_, int nH, int N);   /* 0 for an unsupported shape */
int sdf_win_attn_large_sew_bwd(const SdfWinAttnSewBwdDesc* d, void* stream);

/* ---- the attention half of an ANN video-swin block as one launch (BASELINE config 3, first stage) -----------------
 * Replaces `SwinTransformerBlock3D.forward_part1` + the shortcut (reference models/STSwinNet/swin_transformer3D_v2.py:272-310, :331)
 * with `WindowAttention3D.forward` (:169-205) inside:
 *   out = x + proj(softmax(normalize(q) normalize(k)^T * logit_scale + bias (+ mask)) v),  q | k | v = LayerNorm(x) Wqkv^T + qkv_bias
 * over the windows `row_map` describes (the table of sdf_window_slice_map: row_map[b_ * N + n] = row of token n of window b_ in the
 * (rows, C) tensors, -1 = a padding token: a zero row behind the norm, its output dropped).  q | k | v never exist in memory.
 * Built for C = 96, nH = 3, N = 162 (sdf_ann_attn_block_supported); other shapes: SDF_E_SHAPE, the caller keeps
 * sdf_layer_norm_fwd + sdf_dense_linear_fwd + sdf_win_attn_fwd + sdf_dense_linear_fwd.  x == out is allowed (windows are disjoint).
 * wqkv: fp16 planes [2][3C][C] with W = plane0 + plane1 (plane0 = fp16(W), plane1 = fp16(W - plane0)), rows in the module's
 * order (q | k | v).  wproj: fp16 planes [2][C][C] of the projection weight with the input channels of every head g in the
 * kernel's accumulator order: wproj[., o, 32 g + 8 a + i] = Wproj[o, 32 g + (i < 4 ? 4 a + i : 16 + 4 a + i - 4)], a = 0..3, i = 0..7. */
typedef struct SdfAnnAttnBlockDesc {
  const float* x;            /* (rows, C) */
  float* out;                /* (rows, C) */
  const int32_t* row_map;    /* (B_ * N) */
  int32_t B_, nW, nH, N, C;
  int64_t rows;
  const float* ln_w;         /* (C) */
  const float* ln_b;         /* (C) */
  float ln_eps;
  const uint16_t* wqkv;      /* fp16 planes [2][3C][C] */
  const float* qkv_bias;     /* (3C) or NULL */
  const float* scale;        /* (nH): exp(min(logit_scale, ln 100)) * log2(e) */
  const float* table;        /* (nW, nH, N, N): (16 sigmoid(cpb_mlp(...))[h] + mask[w]) * log2(e), combined once per parameter version
                              * (nW = 1 and no mask for un-shifted windows): the softmax runs in the log2 domain and the score's
                              * additions are the matrix pipe's accumulator input */
  const uint16_t* wproj;     /* fp16 planes [2][C][C], input channels permuted (above) */
  const float* proj_bias;    /* (C) or NULL */
} SdfAnnAttnBlockDesc;

int sdf_ann_attn_block_supported(int C, int nH, int N);
int sdf_ann_attn_block_fwd(const SdfAnnAttnBlockDesc* d, void* stream);

/* ---- the MLP half of an ANN video-swin block as one launch (BASELINE config 3, first stage) ---------------------------
 * Replaces `SwinTransformerBlock3D.forward_part2` + the shortcut (reference models/STSwinNet/swin_transformer3D_v2.py:312-336) with
 * `Mlp.forward` (:15-34) inside:  out = x + fc2(GELU(fc1(LayerNorm(x)))), erf-form GELU (F.gelu), on rows x (rows, C) fp32; the hidden
 * activations never exist in memory.  Built for C = 96, hidden 384 (sdf_ann_mlp_block_supported); other shapes: SDF_E_SHAPE, the caller
 * keeps sdf_layer_norm_fwd + sdf_dense_linear_fwd (GELU) + sdf_dense_linear_fwd (shortcut).  x == out is allowed.
 * w1: fp16 planes [2][Ch][C] of fc1's weight (plane0 = fp16(W), plane1 = fp16(W - plane0)); w2: fp16 planes [2][C][Ch] of fc2's weight
 * with the hidden channels of every group of 32 in the kernel's accumulator order: w2[., o, 32 g + 8 a + i] =
 * W2[o, 32 g + (i < 4 ? 4 a + i : 16 + 4 a + i - 4)], a = 0..3, i = 0..7. */
typedef struct SdfAnnMlpBlockDesc {
  const float* x;            /* (rows, C) */
  float* out;                /* (rows, C) */
  int64_t rows;
  int32_t C, Ch;
  const float* ln_w;         /* (C) */
  const float* ln_b;         /* (C) */
  float ln_eps;
  const uint16_t* w1;        /* fp16 planes [2][Ch][C] */
  const float* b1;           /* (Ch) or NULL */
  const uint16_t* w2;        /* fp16 planes [2][C][Ch], hidden channels permuted (above) */
  const float* b2;           /* (C) or NULL */
} SdfAnnMlpBlockDesc;

int sdf_ann_mlp_block_supported(int C, int Ch);
int sdf_ann_mlp_block_fwd(const SdfAnnMlpBlockDesc* d, void* stream);

/* ---- dense 3x3 convolution of real-valued activations (ANN patch embedding, BASELINE config 3) ----------------------
 * Replaces the library convolutions of reference models/STSwinNet/PatchEmbed.py:166-196 (`PatchEmbedLocal`: head Conv2d +
 * four `ResidualBlock`s, models/submodules.py:160-229) together with their BatchNorm2d (eval: folded to alpha / beta), residual
 * add and ReLU:  out = act(alpha[n] * conv3x3(x, w)[n] + beta[n] (+ resid)), stride 1, zero padding 1.
 * Activations are "planes": [imgs][ceil(C/16)][H][W] records of 64 bytes, a record = 4 pieces of { 4 x fp16 hi, 4 x fp16 lo }
 * for 16 channels (value = hi + lo, 22 significant bits; sdf_pack_planes / sdf_unpack_planes convert from / to NCHW fp32).
 * w: fp16 planes [2][N][K] with w = plane0 + plane1, K = 9 * 16 * cin_records ordered (record, ky, kx, channel in record);
 * channels beyond Cin carry zero weights.  N % 32 == 0; cin_records in {1, 6}; every tensor below 2^31 bytes. */
typedef struct SdfDenseConvDesc {
  const void* x;            /* planes [imgs][cin_records][H][W][64 B] */
  const uint16_t* w;        /* fp16 planes [2][N][K] */
  const float* alpha;       /* (N) or NULL = 1 */
  const float* beta;        /* (N) or NULL = 0 */
  const void* resid;        /* planes [imgs][N/16][H][W][64 B] or NULL */
  void* out;                /* planes [imgs][N/16][H][W][64 B], or fp32 NHWC (imgs,H,W,N) when out_f32 */
  int32_t imgs, H, W, cin_records, N;
  int32_t relu;             /* max(., 0) after the residual add */
  int32_t out_f32;
  int32_t x_records;        /* records per image of the tensor x points into when x is a channel slice of a wider planes tensor
                             * (x = base + first_record * H * W * 64 bytes); 0 = cin_records.  Wide convolutions are chains of
                             * slices: out_k = conv(slice_k) + out_{k-1} through `resid`, the last link carries beta and relu */
  float acc_scale;          /* the planes hold scale * w (scale a power of two chosen at pack time so that max|w| fills the fp16
                             * range: small weights keep their 22 bits instead of sinking into fp16 subnormals); the accumulator is
                             * multiplied by acc_scale = 1 / scale (folded into alpha: exact).  0 = 1 */
} SdfDenseConvDesc;

int sdf_dense_conv3x3_fwd(const SdfDenseConvDesc* d, void* stream);
/* x (imgs,C,H,W) fp32 -> planes (channels C .. 16*ceil(C/16)-1 zero) and back */
int sdf_pack_planes(const float* x, void* planes, int imgs, int C, int H, int W, void* stream);
int sdf_unpack_planes(const void* planes, float* x, int imgs, int C, int H, int W, void* stream);
/* bilinear x2 upsampling (align_corners false; reference models/submodules.py:117-157 `UpsampleConvLayer`) of x (imgs,C,h,w) fp32
 * with element strides (sn,sc,sh,sw), written as records rec0 .. rec0+ceil(C/16)-1 of planes [imgs][rec_total][2h][2w] */
int sdf_pack_planes_up2(const float* x, void* planes, int imgs, int C, int h, int w, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                        int rec0, int rec_total, void* stream);
/* round 6: the same record addressing with ZERO INSERTION instead of interpolation - output pixel (2k, 2l) = input (k, l), all other
 * pixels 0: the input of ConvTranspose2d(3, stride 2, padding 1, output_padding 1) as the stride-1 correlation sdf_dense_conv3x3_fwd
 * runs with the flipped kernel (the SEW decoders, reference Spiking_modules.py:449-456), without a zero-filled fp32 image in between. */
int sdf_pack_planes_zero_up2(const float* x, void* planes, int imgs, int C, int h, int w, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                             int rec0, int rec_total, void* stream);

/* ---- Linear layer on real-valued activations (ANN swin blocks, BASELINE config 3) --------------------------------
 * Replaces F.linear (+ F.gelu, + the residual add) of reference models/STSwinNet/swin_transformer3D_v2.py:176-202
 * (`WindowAttention3D`: qkv, proj), :15-34 (`Mlp`: fc1 -> GELU -> fc2) and :272-313 (the block's two shortcut adds):
 *   out[m, n] = act(sum_k a[m, k] * w[n, k] + bias[n]) (+ resid[m, n]),  act = erf-form GELU when `gelu`, else identity.
 * a, resid, out: fp32 row-major (M, K) / (M, N); out may alias resid.  w: fp16 planes [2][N][K], w = plane0 + plane1
 * (hi = fp16(s w), lo = fp16(s w - hi), s = 1 / acc_scale).  N % 96 == 0, K % 32 == 0, every tensor below 2^31 bytes.
 * Activations are split into hi + lo fp16 in the loader: a value beyond the fp16 range (|x| > 65504) or a NaN becomes inf / NaN
 * and the affected outputs come out NaN - it is never silently replaced by a finite number. */
typedef struct SdfDenseLinearDesc {
  const float* a;
  const uint16_t* w;
  const float* bias;        /* (N) or NULL */
  const float* resid;       /* (M, N) or NULL */
  float* out;
  int32_t M, N, K;
  int32_t gelu;
  /* convolution form (cv_C > 0; all zero = plain Linear): `a` is a channels-last image (imgs, cv_H, cv_W, cv_C) fp32 and row m =
   * (img, oy, ox) gathers the 3x3 / pad 1 / stride cv_stride neighbourhood, K = 9 * cv_C ordered (ky, kx, c) - the strided
   * projection of reference models/STSwinNet/PatchEmbed.py:191 (`PatchEmbedLocal.proj`).  cv_OH / cv_OW = (H - 1) / stride + 1;
   * out_T > 1 writes image t * B + b of the input as image b * out_T + t of the output ((T,B) -> (B,T): the layout the swin
   * stages consume).  No residual in this form. */
  int32_t cv_H, cv_W, cv_C, cv_stride, cv_OH, cv_OW, out_T;
  float acc_scale;          /* 1 / (power-of-two scale the weight planes were packed with); multiplies the accumulator before the
                             * bias (exact).  0 = 1 */
} SdfDenseLinearDesc;

int sdf_dense_linear_fwd(const SdfDenseLinearDesc* d, void* stream);

/* Weight gradient of a Linear layer fed by spikes (training path, BASELINE configs[3]): dw[n, k] = sum_m dy[m, n] * x[m, k] - what
 * autograd computes for every nn.Linear of the MS swin blocks in the reference's step (train_flow_parallel_supervised_SNN.py:233-336
 * `loss.backward()`; layers Spiking_swin_transformer3D.py:661-717, :164-181, :952-974).  dy (M, N) and x (M, K) fp32 row-major, x
 * holding values exact in bf16 (spikes: 0 / 1); dy is split into three bf16 planes inside the kernel (exact), fp32 accumulation.
 * N % 96 == 0, K % 96 == 0.  nsplit = sdf_linear_dw_splits(M, N, K, cv_C) ranges of m are summed in a fixed order through `partial`
 * (nsplit x N x K fp32; may be NULL when nsplit == 1).  dw is overwritten.
 *
 * Convolution form (cv_C > 0): the weight gradient of a 3x3 / stride 1 / pad 1 convolution fed by spikes (the patch embedding's and
 * the bottleneck's MS_ResBlock convolutions, reference Spiking_modules.py:291-347; autograd's `conv2d_weight`) on ZERO-RINGED
 * channels-last images: row m is a pixel of the (H + 2) x cv_Wp grid of an image (cv_Wp = W + 2), dy (M, N) is zero on the ring, x is
 * (M, cv_C) with the ring zero (the convolution's padding), K = 9 cv_C and
 *   dw[n, (ky * 3 + kx) * cv_C + c] = sum_m dy[m, n] * x[m + (ky - 1) * cv_Wp + (kx - 1), c]       (rows outside [0, M) read as zero)
 * cv_C % 96 == 0. */
typedef struct SdfLinearDwDesc {
  const float* dy;
  const float* x;
  float* dw;
  float* partial;
  int64_t M;
  int32_t N, K, nsplit;
  int32_t cv_C, cv_Wp;
} SdfLinearDwDesc;

int sdf_linear_dw_splits(int64_t M, int N, int K, int cv_C);
int sdf_linear_dw_fwd(const SdfLinearDwDesc* d, void* stream);
/* src (imgs, C, H, W) fp32 -> dst (imgs, H + 2, W + 2, C) fp32, the ring zero: the layout of the convolution form above.  C % 96 == 0. */
int sdf_ringed_rows_fwd(const float* src, float* dst, int imgs, int C, int H, int W, void* stream);
/* the way back: src (imgs, H + 2, W + 2, C) ringed channels-last rows -> dst (imgs, C, H, W), + bias[c] when bias != NULL.  C % 96 == 0. */
int sdf_unring_rows_fwd(const float* src, const float* bias, float* dst, int imgs, int C, int H, int W, void* stream);

/* The two activation-side products of a Linear layer in the training path, from the fp32 tensors autograd holds (reference: nn.Linear
 * forward / autograd in train_flow_parallel_supervised_SNN.py:233-336; layers Spiking_swin_transformer3D.py:661-717, :164-181, :952-974):
 *   mode 0  out (M, N) = a (M, K) * w^T + bias     a holds spikes (values exact in bf16), w (N, K) fp32;   K % 32 == 0, N % 96 == 0
 *   mode 1  out (M, K) = a (M, N) * w              a = dY fp32 (any range), w (N, K) fp32;                 N % 32 == 0, K % 96 == 0
 * Real operands are split into three bf16 planes inside the kernel (exact; fp32 exponent range), fp32 accumulation.  bias: mode 0 only,
 * may be NULL.
 * Convolution form of mode 0 (cv_C > 0): the FORWARD of a 3x3 / stride 1 / pad 1 convolution fed by spikes (MS_ResBlock, reference
 * Spiking_modules.py:291-347) on the zero-ringed channels-last pixel rows of sdf_ringed_rows_fwd: a is (M, cv_C), w is (N, 9 cv_C) ordered
 * (ky, kx, c) [= weight.permute(0, 2, 3, 1)], K = 9 cv_C, out (M, N) on the same ringed grid (ring rows hold no result: sdf_unring_rows_fwd
 * drops them on the way back to NCHW). */
typedef struct SdfLinearTrainDesc {
  const float* a;
  const float* w;
  const float* bias;
  float* out;
  int32_t M, N, K;
  int32_t mode;
  int32_t cv_C, cv_Wp;
} SdfLinearTrainDesc;

int sdf_linear_train_fwd(const SdfLinearTrainDesc* d, void* stream);

/* nn.LayerNorm over the last dim of x (rows, C) fp32, elementwise affine (reference models/STSwinNet/swin_transformer3D_v2.py:
 * `norm1` / `norm2` of the blocks :231-233, `PatchMerging.norm` :356, the per-stage output norms :622-624).  C % 4 == 0, C <= 2048. */
int sdf_layer_norm_fwd(const float* x, const float* gamma, const float* beta, float* out, int64_t rows, int C, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Raw event lists -> voxel grid: the front end the model's input comes from when the data is not preprocessed.
 * Replaces: VoxelGrid.convert_CHW / convert_CHW_polarities (reference DSEC_dataloader/event_representations.py:241-313), optionally with
 * rectify_events (:20-28) in front and the input preparation of the evaluation loop behind (eval_DSEC_flow_SNN.py:179-217: centre crop,
 * polarity split, min-max over the non-zeros, spike threshold).  Semantics are the reference's, quirks included:
 *   t_norm = (C - 1) (t - t[0]) / (t[N-1] - t[0])  fp32, multiply then divide;  x0, y0, t0 = truncation toward zero;
 *   the 8 corners (x0 | x0+1, y0 | y0+1, t0 | t0+1), kept iff inside [0, W) x [0, H) x [0, C);
 *   weight (2p - 1) (1 - |xc - x|) (1 - |yc - y|) (1 - |tc - t_norm|), three fp32 products in that order (negative for x in (-1, 0));
 *   a cell's sum is formed in the order of the reference's CPU put_: corner passes x outer / y middle / t inner, list order inside a pass.
 * No float atomics: results are bit-identical from run to run and do not depend on how the lists are batched.
 *
 * B event lists lie back to back in x, y, t, p (n_events in all); `offsets` is a HOST array of B + 1 positions (NULL: B == 1).  A list
 * is in time order; an empty list gives a zero grid.  A list with t[last] == t[first] has no t_norm (the reference returns NaN): pass
 * the HOST array t_range = {t_first, t_last} per list and the call is refused with SDF_E_SHAPE before any launch; with t_range NULL it
 * is not detected and that list's events add nothing.
 * xy_dtype 0: x, y fp32 (already rectified, possibly fractional).  1 / 2: int32 / uint16 sensor coordinates, looked up in
 * rectify_map (map_h, map_w, 2) fp32 as x, y <- map[y, x]; an event outside the map adds nothing.
 * crop_h, crop_w > 0: only the centre window (crop_h, crop_w) of the (H, W) grid is computed and written; 0, 0: the whole grid.
 * mode 0: out = the signed grid (B, C, h, w).
 * mode 1: out = the model's input (B, C, 2, h, w): relu(v) | relu(-v); norm 1 = min-max over the non-zero elements of the whole output;
 *         use_spike_th: > spike_th -> 1, < spike_th -> 0 (sdformerflow_amd.harness.prepare_chunk).  norm / use_spike_th: mode 1 only.
 * mode 2: out = convert_CHW_polarities (B, C, 2, h, w): unsigned weights of the p == 1 | p == 0 events.
 *
 * Two calls with the caller's stable sort between them (the sort is plumbing: any stable sort of int32 keys):
 *   sdf_event_voxel_keys_fwd    writes keys[n_events] (the event's base-cell key; events that touch no output cell sort last)
 *   caller                      keys_sorted, order = stable ascending sort of keys (order: int64 positions into the event arrays)
 *   sdf_event_voxel_gather_fwd  out, from keys_sorted, order and the workspace the first call filled
 * workspace: sdf_event_voxel_workspace_bytes(...) bytes, 16-byte aligned, the same for both calls (0: refused geometry). */
typedef struct SdfEventVoxelDesc {
  const void* x;
  const void* y;
  const float* t;
  const float* p;
  const float* rectify_map;
  const int64_t* offsets;
  const float* t_range;
  int32_t* keys;
  const int32_t* keys_sorted;
  const int64_t* order;
  void* out;
  void* workspace;
  int64_t workspace_bytes, n_events;
  int32_t B, C, H, W, crop_h, crop_w, map_h, map_w;
  int32_t xy_dtype, mode, norm, use_spike_th;
  float spike_th;
} SdfEventVoxelDesc;

int64_t sdf_event_voxel_workspace_bytes(int64_t n_events, int B, int C, int H, int W, int crop_h, int crop_w);
int sdf_event_voxel_keys_fwd(const SdfEventVoxelDesc* d, void* stream);
int sdf_event_voxel_gather_fwd(const SdfEventVoxelDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Raw event lists -> the time-bilinear voxel grid of the MVSEC / MDR loaders, and the model's input behind it.
 * Replaces: EventSequence(..., timestamp_multiplier, convert_to_relative=True) + EventSequenceToVoxelGrid_Pytorch (reference
 * MDR_dataloader/loader_utils.py:344-389, 421-577) and the input preparation of eval_MV_flow_SNN.py:162-219 (old | new along the bins,
 * polarity split, min-max over the non-zeros, spike threshold, event mask).  Semantics are the reference's, per list:
 *   ts = t * t_scale - (t * t_scale)[0];  deltaT = ts[last] (1.0 if that is 0);  tn = (nb - 1) * ts / deltaT, all float64, multiply
 *   then divide;  tis = floor(tn);  dts = fp32(tn - tis);  x, y truncated to integers;  pol = p with 0 -> -1;
 *   left pass: grid[tis, y, x] += pol * (1 - dts) for 0 <= tis < nb;  right pass: grid[tis + 1, y, x] += pol * dts for tis + 1 < nb;
 *   a cell sums its left-pass events in list order, then its right-pass events in list order, in fp32 (index_add_ on the CPU);
 *   normalize: over the non-zero cells of the list's WHOLE (nb, H, W) grid, v <- (v - mean) / std (unbiased std; v - mean when std is
 *   not > 0; nothing without a non-zero cell).  mean and std are fp64 sums combined in a fixed order, the quotient is formed in fp64
 *   and rounded once.
 * No float atomics: results are bit-identical from run to run and do not depend on how the lists are batched.
 * Unlike the reference: an event with x outside [0, W) or y outside [0, H) adds nothing (the reference writes into a neighbouring row
 * or bin, or raises); a list whose times are all equal goes to bin 0 with weight pol (its deltaT = 1.0 rule); an empty list gives zeros.
 *
 * n_lists event lists lie back to back in x, y, t, p (n_events in all, each list in time order); `offsets` is a HOST array of
 * n_lists + 1 positions.  t is float64; `t_scale` is a HOST pointer to the float64 multiplier (NULL: 1.0).  xy_dtype 0 / 1 / 2: x, y
 * fp32 / int32 / uint16.  crop_h, crop_w > 0: only the window (crop_h, crop_w) at (crop_oy, crop_ox) is written - and, without
 * normalize, computed; 0, 0 (origin 0, 0): the whole grid.
 * mode 0: out = the signed volumes (n_lists, nb, h, w).
 * mode 1: out = the model's input (n_lists / lists_per_sample, lists_per_sample * nb, 2, h, w): the lists of a sample (old, new) one
 *         after the other along the bins, relu(v) | relu(-v); norm 1 = min-max over the non-zero elements of the whole output;
 *         use_spike_th: > spike_th -> 1, < spike_th -> 0; event_mask (may be NULL): (samples, 1, h, w) fp32, 1 where any element of the
 *         pixel is non-zero.  lists_per_sample 1 | 2; norm / use_spike_th / event_mask / lists_per_sample 2: mode 1 only.
 * mode 2: out = the pol=False form (n_lists, nb, 2, h, w): unsigned weights of the pol == 1 | pol == -1 events.
 *
 * Two calls with the caller's stable sort between them, as for sdf_event_voxel_*:
 *   sdf_event_voxel_tb_keys_fwd    writes keys[n_events]
 *   caller                         keys_sorted, order = stable ascending sort of keys (order: int64 positions into the event arrays)
 *   sdf_event_voxel_tb_gather_fwd  out (and event_mask)
 * workspace: sdf_event_voxel_tb_workspace_bytes(...) bytes, 16-byte aligned, the same for both calls (0: refused geometry). */
typedef struct SdfEventVoxelTbDesc {
  const void* x;
  const void* y;
  const double* t;
  const double* t_scale;
  const float* p;
  const int64_t* offsets;
  int32_t* keys;
  const int32_t* keys_sorted;
  const int64_t* order;
  void* out;
  float* event_mask;
  void* workspace;
  int64_t workspace_bytes, n_events;
  int32_t n_lists, lists_per_sample, nb, H, W, crop_h, crop_w, crop_oy, crop_ox;
  int32_t xy_dtype, normalize, mode, norm, use_spike_th;
  float spike_th;
} SdfEventVoxelTbDesc;

int64_t sdf_event_voxel_tb_workspace_bytes(int64_t n_events, int n_lists, int nb, int H, int W, int crop_h, int crop_w, int crop_oy, int crop_ox, int normalize);
int sdf_event_voxel_tb_keys_fwd(const SdfEventVoxelTbDesc* d, void* stream);
int sdf_event_voxel_tb_gather_fwd(const SdfEventVoxelTbDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Raw event lists + an estimated flow -> the image of warped events (IWE): every event is moved along the flow of its pixel to a common
 * time and accumulated per polarity.  The ground-truth-free view of a flow's quality (the reference's Visualization_DSEC has `iwe`
 * slots its loops leave None: there is no reference implementation; this text is the definition).
 * Per event, in fp32, every operation rounded on its own:
 *   tn = (t - t_first) / (t_last - t_first) of its list; skipped unless win_a <= tn <= win_b (NaN fails); tau = (tn - win_a) / (win_b - win_a);
 *   lookup pixel xi = (int)floorf(x + 0.5f) - ox, yi likewise; skipped outside [0, w) x [0, h);
 *   u = scale * flow[b, 0, yi, xi], v = scale * flow[b, 1, yi, xi]; skipped if either is not finite;
 *   d = t_ref - tau;  xw = (x - ox) + d * u;  yw = (y - oy) + d * v;  channel 0 if p > 0, else 1;
 *   mode 0 (bilinear): x0 = floorf(xw), y0 = floorf(yw); corner (x0 + dx, y0 + dy) gets (1 - |xc - xw|) * (1 - |yc - yw|), corners
 *     outside the window are dropped; a cell's sum is formed in the order: passes dx outer, dy inner, list order within a pass;
 *   mode 1 (nearest): weight 1 at (rintf(xw), rintf(yw)), halves to even, -0 = 0, dropped outside: the image holds integers.
 * out (B, 2, h, w) fp32; flow (B, 2, h, w) fp32 on the same window: (crop_h, crop_w) at (crop_oy, crop_ox) of the (H, W) sensor, or the
 * whole sensor (all four 0).  An empty list gives zeros.  No float atomics: bit-identical from run to run, and a list's image does not
 * depend on its batch.  Event arrays, offsets (HOST), t_range (HOST), xy_dtype and rectify_map: as SdfEventVoxelDesc.
 * Two calls with the caller's stable sort between them, as for sdf_event_voxel_*; workspace: sdf_event_iwe_workspace_bytes(...) bytes,
 * 16-byte aligned, the same for both calls (0: refused geometry or mode).
 * Checks, before any launch: SDF_E_NULL: d, flow, out, workspace (x, y, t, p, keys / keys_sorted, order with events; offsets with
 * B > 1; an integer xy_dtype without its map); SDF_E_SHAPE: a refused geometry, not win_a < win_b, a value that is not finite, a short
 * workspace, offsets that do not cut n_events, a list with t_last == t_first in t_range; SDF_E_DTYPE: mode outside 0 | 1, xy_dtype
 * outside 0 .. 2, a map with fp32 coordinates - and, last, a pointer the kernels would read or write that is not device memory;
 * SDF_E_ALIGN: workspace not 16-byte, an fp32 / int32 pointer not 4-byte, a uint16 pointer not 2-byte, order not 8-byte aligned.
 * Added to SDF_VERSION 107 (no existing entry changed). */
typedef struct SdfEventIweDesc {
  const void* x;
  const void* y;
  const float* t;
  const float* p;
  const float* flow;
  const float* rectify_map;
  const int64_t* offsets;
  const float* t_range;
  int32_t* keys;
  const int32_t* keys_sorted;
  const int64_t* order;
  void* out;
  void* workspace;
  int64_t workspace_bytes, n_events;
  int32_t B, H, W, crop_h, crop_w, crop_oy, crop_ox, map_h, map_w;
  int32_t xy_dtype, mode;
  float scale, t_ref, win_a, win_b;
} SdfEventIweDesc;

int64_t sdf_event_iwe_workspace_bytes(int64_t n_events, int B, int H, int W, int crop_h, int crop_w, int crop_oy, int crop_ox, int mode);
int sdf_event_iwe_keys_fwd(const SdfEventIweDesc* d, void* stream);
int sdf_event_iwe_gather_fwd(const SdfEventIweDesc* d, void* stream);

/* sdf_iwe_stats_fwd: sample b of iwe (B, 2, H, W) fp32 writes row row0 + b of `table` (double[rows][4]; other rows stay):
 *   {sum c, sum c^2, max c, number of pixels with c != 0},  c = the fp64 sum of the pixel's two channels
 * fp64 sums formed lane -> wave -> workgroup -> one partial record per workgroup in the workspace, then combined per sample in index
 * order: no atomics, bit-identical from run to run and independent of B.  On nearest images the sums are integers, exact below 2^53; the
 * Flow Warp Loss of a sample is var(S) / var(Z), var = (sum c^2 - (sum c)^2 / N) / (N - 1) over the N = H W pixels, S the image warped
 * by the flow and Z the one with scale 0.
 * workspace: sdf_iwe_stats_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: refused geometry).
 * SDF_E_NULL: d, iwe, table or workspace NULL; SDF_E_SHAPE: B, H or W < 1, B > 65535, H W >= 2^30, rows outside the table, a short
 * workspace; SDF_E_ALIGN: iwe not 4-byte, table or workspace not 8-byte aligned; SDF_E_DTYPE: a pointer that is not device memory. */
typedef struct SdfIweStatsDesc {
  const float* iwe;
  double* table;
  void* workspace;
  int64_t workspace_bytes;
  int32_t B, H, W, row0, rows;
} SdfIweStatsDesc;

int64_t sdf_iwe_stats_workspace_bytes(int B, int H, int W);
int sdf_iwe_stats_fwd(const SdfIweStatsDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Flow maps -> the per-sample sums of the evaluation metrics (reference loss/flow_supervised.py: AEE :119-149, AAE :163-175).
 * pred, label (B, 2, H, W), valid (B, H, W), event_mask (B, H, W; may be NULL): fp32, contiguous.  Per pixel, every step one fp32
 * operation in the reference's order, constants Python doubles rounded to fp32:
 *   f = pred * flow_scaling;  m = valid [* event_mask];  e = sqrt((fx - lx)^2 + (fy - ly)^2) * m;  mag = sqrt(fx^2 + fy^2) * m;
 *   gm = sqrt(lx^2 + ly^2) * m;  cos = clamp((fx lx + fy ly + 1e-7) / (mag * gm + 1e-7), -1 + 1e-7, 1 - 1e-7);  ang = acosf(cos) * m.
 * Sample b writes row row0 + b of `table` (double[rows][8]; every other row is left as it is):
 *   {n_valid = sum m, sum_err = sum e, n_pe1 = #(e > 1), n_pe2 = #(e > 2), n_pe3 = #(e > 3), n_outlier = #(e > 3 && e > 0.05f * mag),
 *    sum_ang = sum ang, n_pixels = H W}
 * with integer counts and fp64 sums of the fp32 values, formed lane -> wave -> workgroup -> one partial record per workgroup in the
 * workspace, then added per sample in index order: no float atomics, bit-identical from run to run and independent of B.  A sample's
 * record is that of a batch-1 call of the classes; their batch-coupled forms at B > 1 (`outliers.sum()` over the whole batch, the
 * (B, 1, H, W) * (B, H, W) broadcast of AAE) are not reproduced.
 * workspace: sdf_flow_metrics_workspace_bytes(B, H, W) bytes, 8-byte aligned (0: refused geometry). */
typedef struct SdfFlowMetricsDesc {
  const float* pred;
  const float* label;
  const float* valid;
  const float* event_mask;
  double* table;
  void* workspace;
  int64_t workspace_bytes;
  int32_t B, H, W, row0, rows;
  float flow_scaling;
} SdfFlowMetricsDesc;

int64_t sdf_flow_metrics_workspace_bytes(int B, int H, int W);
int sdf_flow_metrics_fwd(const SdfFlowMetricsDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder predictions of every level -> the supervised multi-scale flow loss (reference loss/flow_supervised.py:85-102, gamma None)
 * and its gradient at each level's own resolution: the training twin of the metrics above.  Added to SDF_VERSION 107 (no existing entry
 * changed).  `levels` (1 .. SDF_FLOW_LOSS_MAX_LEVELS) predictions; level i: pred[i] (T[i], B, 2, h[i], w[i]) contiguous, of `dtype`
 * (SDF_FLOW_LOSS_F32 / _BF16 / _F16, one for all levels), T[i] in 1 .. 64, factor s = H / h[i] = W / w[i] in {1, 2, 4, 8, 16} - the
 * factors at which F.interpolate's nearest index floor(dst * (1 / s)) in fp32 equals dst / s.  label (B, 2, H, W), mask (B, H, W) fp32
 * (the caller's mask * event_mask); n_valid: one fp32 on the device (the valid-pixel count the errors are divided by, all-reduced or
 * not).  At full-resolution pixel (Y, X), every step one fp32 operation, constants Python doubles rounded to fp32:
 *   f = sum_t pred[i][t][b][c][Y / s][X / s]   (t ascending; 16-bit inputs: rounded once to the input type when T > 1)
 *   d = f * flow_scaling - label;  r = sqrtf(dx dx + dy dy + 1e-8);  err = r * m          (the mask multiplies, it does not select)
 *   S[i][b] = sum err over the sample, an fp64 sum of the fp32 values -> records[i * B + b] (records may be NULL)
 *   loss[0] = mean_b sum_i lambda_mod S[i][b] / (n_valid + 1e-9) / levels, in fp64 with n_valid + 1e-9 formed in fp32, rounded once
 *   grad[i] (B, 2, h[i], w[i]) fp32 = the sum over the s x s block, row-major, of m * d_c / r * k,
 *     k = fp32(flow_scaling lambda_mod / (levels B)) / (n_valid + 1e-9): d loss / d f at the level's resolution.
 * grad[i] is given for every level or for none (loss only).  One partial launch over 16 x 64 tiles of the frame and one finish launch,
 * whatever `levels`; label and mask are read once; no float atomics; every output element is written once; bit-identical from run to
 * run, and a sample's records depend on that sample alone.
 * workspace: as many bytes as sdf_flow_loss_workspace_bytes returns for (B, H, W, levels), 8-byte aligned (0: refused geometry - B
 * outside 1 .. 65535, H W >= 2^30, levels outside 1 .. 8). */
#define SDF_FLOW_LOSS_MAX_LEVELS 8
#define SDF_FLOW_LOSS_F32 0
#define SDF_FLOW_LOSS_BF16 1
#define SDF_FLOW_LOSS_F16 2

typedef struct SdfFlowLossDesc {
  const void* pred[8];
  float* grad[8];
  int32_t h[8], w[8], T[8];
  const float* label;
  const float* mask;
  const float* n_valid;
  float* loss;
  double* records;
  void* workspace;
  int64_t workspace_bytes;
  int32_t levels, B, H, W, dtype;
  float flow_scaling, lambda_mod;
} SdfFlowLossDesc;

int64_t sdf_flow_loss_workspace_bytes(int B, int H, int W, int levels);
int sdf_flow_loss_fwd(const SdfFlowLossDesc* d, void* stream);

/* the largest batch of one sdf_augment_chunk_fwd / sdf_augment_resize_fwd call: their per-sample arrays travel as kernel arguments */
#define SDF_AUGMENT_MAX_B 64

/* ---------------------------------------------------------------------------------------------
 * An MDR loader item -> the training step's (input, label, mask): the reference's DenseSparseAugmentor (MDR_dataloader/loader_utils.py:
 * 244-341; MDR.py:218-241) - bilinear rescale, flow * scale, flips, crop, valid mask - followed by the loop's cat((old, new), dim=1),
 * polarity split and preparation (train_mdr_supervised_SNN.py:209-276), with the random decisions drawn by the caller.
 * Added to SDF_VERSION 107 (no existing entry changed).
 * vox_old, vox_new (B, bins, Hs, Ws) fp32 signed (the loader's d_event_volume_old / _new; vox_old may be NULL when num_chunks is 1 and is
 * not read then), flow (B, 2, Hs, Ws) fp32.  Per sample b (host arrays, B <= SDF_AUGMENT_MAX_B entries used; scale_x / scale_y point
 * at B host doubles, read during the call): resized[b]; the scales; the resized size rh[b], rw[b] = rint(Hs scale_y), rint(Ws scale_x)
 * (half to even), or (Hs, Ws) when not resized; flags[b] bit 0 horizontal, bit 1 vertical flip; the crop origin oy[b], ox[b] in the
 * flipped, resized image.  Order, as the reference: resize, horizontal flip, vertical flip, crop.
 *   output pixel (y, x) lies at (oy + y, ox + x) of the flipped image = (vflip ? rh-1-(oy+y) : oy+y, hflip ? rw-1-(ox+x) : ox+x) of the
 *   resized one.  Each axis maps that index d as cv2.resize(INTER_LINEAR) does for a source of n elements: c = (float)((d + 0.5) / scale
 *   - 0.5) with 1 / scale, the product and the difference in double; i = floor(c), a = c - i in float; i < 0: i = 0, a = 0;
 *   i >= n - 1: i = n - 1, a = 0; second tap min(i + 1, n - 1).  value = (S[y0][x0] (1 - ax) + S[y0][x1] ax) (1 - ay) + (S[y1][x0]
 *   (1 - ax) + S[y1][x1] ax) ay, every product and sum rounded to fp32 on its own: bit for bit the numpy restatement
 *   (MDR_dataloader.loader_utils.resize_linear).  A real cv2 build may contract the vertical pass: unchecked.  resized[b] == 0: the one
 *   source pixel, copied.
 *   label_out (B, 2, h, w) = (float)((double)value * scale * sign), sign -1 for the x component under a horizontal and the y component
 *   under a vertical flip, scale 1 when not resized;
 *   mask_out (B, 1, h, w) fp32 = !isinf(u) && !isinf(v) && sqrt(u u + v v) > 0 on those doubles before the rounding (a NaN, and two
 *   zeros, give 0).  The reference evaluates the norm in fp32 for an item that is neither resized nor flipped, where components below
 *   about 1e-23 underflow to "invalid"; the double rule is used throughout here;
 *   out (B, nF, 2, h, w), nF = num_chunks * bins, the old volume's bins first = relu(v) | relu(-v), then norm / per_sample /
 *   use_spike_th / event_mask as SdfPrepareChunkDesc; mask_events: mask_out is multiplied by the event mask.
 * Launches: [clear the min / max pairs] | gather + split | [finish]; nothing is allocated, nothing waits for the host.
 * workspace: sdf_augment_resize_workspace_bytes(B) bytes, 8-byte aligned (0: refused B).
 * SDF_E_SHAPE: B outside 1 .. SDF_AUGMENT_MAX_B, a dimension or a crop side < 1, a resized sample whose scale is not finite and positive
 * or whose size is not rint(Hs scale_y) x rint(Ws scale_x), a sample that is not resized with another size than the source's, a size
 * smaller than the crop, an origin outside [0, rh - h] x [0, rw - w] (all checked for every sample before anything is launched), a
 * short workspace; SDF_E_DTYPE: norm outside 0 | 1, num_chunks outside 1 | 2, a flags word with other bits; SDF_E_NULL: d, scale_x,
 * scale_y (the geometry check reads them: refused first), vox_new, flow, out, label_out, mask_out or workspace NULL, vox_old NULL with
 * num_chunks 2; SDF_E_ALIGN: an fp32 pointer not 4-byte or the workspace not 8-byte aligned. */
typedef struct SdfAugmentResizeDesc {
  const float* vox_old;
  const float* vox_new;
  const float* flow;
  const double* scale_x;
  const double* scale_y;
  float* out;
  float* label_out;
  float* mask_out;
  float* event_mask;
  void* workspace;
  int64_t workspace_bytes;
  int32_t B, bins, Hs, Ws, crop_h, crop_w, num_chunks;
  int32_t norm, per_sample, use_spike_th, mask_events;
  float spike_th;
  int32_t resized[64], rh[64], rw[64], oy[64], ox[64], flags[64];
} SdfAugmentResizeDesc;

int64_t sdf_augment_resize_workspace_bytes(int B);
int sdf_augment_resize_fwd(const SdfAugmentResizeDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A loader item -> the training step's (input, label, mask): the reference loops' Compose([RandomCrop, Random_horizontal_flip,
 * Random_vertical_flip, Random_event_drop]) (DSEC_dataloader/data_augmentation.py) followed by the preparation below
 * (train_flow_parallel_supervised_SNN.py:241-308), with the random decisions drawn by the caller and every operation IEEE fp32: the
 * outputs equal the torch composition bit for bit.  Added to SDF_VERSION 107 (no existing entry changed).
 * voxel (B, bins, Hs, Ws) fp32 signed; label (B, 2, Hs, Ws) fp32 and valid (B, 1, Hs, Ws) fp32 or, with valid_is_u8, one byte per
 * element - each may be NULL together with its output.  Per sample b (host arrays, B <= SDF_AUGMENT_MAX_B entries used): the window
 * origin oy[b], ox[b] of the (crop_h, crop_w) window (0, 0: the whole volume, origins 0); flags[b] bit 0 horizontal, bit 1 vertical
 * flip; drop_q[b], negative = no drop.  Order: crop, flips, drop, preparation.
 *   output pixel (y, x) reads the source at (oy + (vflip ? h-1-y : y), ox + (hflip ? w-1-x : x));
 *   label_out (B, 2, h, w): the gathered flow, its x component negated under a horizontal, its y component under a vertical flip;
 *   mask_out (B, 1, h, w) fp32: the gathered valid != 0 as 0.f / 1.f;
 *   drop: v = v * (u > q ? 1.f : 0.f), u = drop_u[cell] when drop_u (B, bins, h, w; output coordinates) is given, else Philox4x32-10
 *     at the cell's linear index i in (B, bins, h, w): key = seed, counter = {i >> 2 (two words), offset (two words)}, the word taken is
 *     number i & 3, u = (word >> 8) * 2^-24;
 *   out (B, bins, 2, h, w) = relu(v) | relu(-v), then norm / per_sample / use_spike_th / event_mask as SdfPrepareChunkDesc;
 *   mask_events: mask_out is multiplied by the event mask (the loops' mask * event_mask, metrics.mask_events).
 * Launches: [clear the min / max pairs] | gather + split | [finish]; nothing is allocated, nothing waits for the host.
 * workspace: sdf_augment_chunk_workspace_bytes(B) bytes, 8-byte aligned (0: refused B).
 * SDF_E_SHAPE: B outside 1 .. SDF_AUGMENT_MAX_B, a dimension < 1, half a crop, a crop larger than the volume, an origin outside
 * [0, Hs - h] x [0, Ws - w] (checked for every sample before anything is launched), a short workspace; SDF_E_DTYPE: norm outside 0 | 1,
 * a flags word with other bits; SDF_E_NULL: d, voxel, out or workspace NULL, label / valid without its output or the reverse,
 * mask_events without mask_out; SDF_E_ALIGN: an fp32 pointer not 4-byte or the workspace not 8-byte aligned. */
typedef struct SdfAugmentChunkDesc {
  const float* voxel;
  const float* label;
  const void* valid;
  const float* drop_u;
  float* out;
  float* label_out;
  float* mask_out;
  float* event_mask;
  void* workspace;
  int64_t workspace_bytes, seed, offset;
  int32_t B, bins, Hs, Ws, crop_h, crop_w;
  int32_t valid_is_u8, norm, per_sample, use_spike_th, mask_events;
  float spike_th;
  int32_t oy[64], ox[64], flags[64];
  float drop_q[64];
} SdfAugmentChunkDesc;

int64_t sdf_augment_chunk_workspace_bytes(int B);
int sdf_augment_chunk_fwd(const SdfAugmentChunkDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Signed voxel volume -> the model's input: harness.prepare_chunk(center_crop(voxel, crop), norm_input, spike_th, polarity=True)
 * (reference eval_DSEC_flow_SNN.py:179-217) with every decision on the device; the output equals the torch composition bit for bit.
 * voxel (B, bins, Hs, Ws) fp32 -> out (B, bins, 2, h, w) = relu(v) | relu(-v) on the window (crop_h, crop_w) at (crop_oy, crop_ox)
 * (0, 0 at origin 0, 0: the whole volume).  norm 1: (v - lo) / (hi - lo) on the non-zeros, lo / hi their min / max (integer atomics on
 * the bit patterns of positive floats: order-independent), when there is a non-zero and lo != hi - over the whole batch tensor
 * (per_sample 0, the reference's semantics) or over each sample (per_sample 1: what B batch-1 calls compute).  norm 0: none; any other
 * value ("std") is refused with SDF_E_DTYPE.  use_spike_th: > spike_th -> 1, < spike_th -> 0.  event_mask (may be NULL): (B, 1, h, w)
 * fp32, 1 where any element of the pixel is non-zero in the result.
 * workspace: sdf_prepare_chunk_workspace_bytes(B) bytes, 8-byte aligned (0: refused B). */
typedef struct SdfPrepareChunkDesc {
  const float* voxel;
  float* out;
  float* event_mask;
  void* workspace;
  int64_t workspace_bytes;
  int32_t B, bins, Hs, Ws, crop_h, crop_w, crop_oy, crop_ox;
  int32_t norm, per_sample, use_spike_th;
  float spike_th;
} SdfPrepareChunkDesc;

int64_t sdf_prepare_chunk_workspace_bytes(int B);
int sdf_prepare_chunk_fwd(const SdfPrepareChunkDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * What was evaluated, as images (reference utils/visualization.py Visualization_DSEC, `vis.store`): bytes into a caller's buffer on
 * the stream, no read-back, nothing allocated.  Added to SDF_VERSION 107 (no existing entry changed).
 *
 * sdf_flow_image_fwd: flow (B, 2, H, W) fp32 [* mask (B, 1, H, W) fp32, multiplied in first; may be NULL] -> out (B, H, W, 3) u8, the
 * reference's flow_to_image of every sample on its own.  Two launches:
 *   1  mag = sqrtf(fx * fx + fy * fy) (np.linalg.norm in fp32: two products, one add, a correctly rounded root); mag >= 0, so its bits
 *      order as unsigned integers: per-sample min / max lane -> wave -> workgroup -> one atomicMin / atomicMax per workgroup into the
 *      sample's two workspace words, which the call itself initialises on the stream.  Order-independent: the same bits on every run.
 *   2  h = (atan2f(fy, fx) + (float)pi) * (float)(1 / pi / 2);  v = (double)(mag - min) / (double)(max - min) (undivided when
 *      max == min);  matplotlib's hsv_to_rgb with s = 1 in fp64 - i = (int)(h * 6), f = h * 6 - i, the six cases of i % 6 (h may be
 *      exactly 1: i = 6 is case 0);  byte = (uint8)(255 * c), truncated.
 * Only atan2f is not bit-equal to numpy's; a byte can differ by one where 255 * c lies within that error of an integer.  NaN flows:
 * the bytes are unspecified, and nothing faults.
 * Loads are 16 bytes per lane where the planes of a sample share their alignment, element-wise in front of the first and behind the
 * last 16-byte boundary and everywhere otherwise; nothing outside the addressed floats is read.  A pixel's three bytes are written by
 * one lane.
 * workspace: sdf_flow_image_workspace_bytes(B, H, W) bytes, 4-byte aligned (0: refused geometry).
 * SDF_E_NULL: d, flow, out or workspace NULL; SDF_E_SHAPE: B, H or W < 1, B > 65535, H W >= 2^30, workspace too small;
 * SDF_E_ALIGN: flow, mask or workspace not 4-byte aligned. */
typedef struct SdfFlowImageDesc {
  const float* flow;
  const float* mask;
  uint8_t* out;
  void* workspace;
  int64_t workspace_bytes;
  int32_t B, H, W;
} SdfFlowImageDesc;

int64_t sdf_flow_image_workspace_bytes(int B, int H, int W);
int sdf_flow_image_fwd(const SdfFlowImageDesc* d, void* stream);

/* sdf_flow_submission_fwd: flow (B, 2, H, W) fp32 -> out (B, H, W, 3) u16 in the DSEC benchmark's encoding (the reference's
 * `flow_test` branch of Visualization_DSEC.store): channels 0 and 1 = (uint16)(f * 128.f + 32768.f) - the product and the sum
 * rounded one by one in fp32, then truncated - and channel 2 = 0.  Bit-exact for |f| < 256 px; beyond that the reference's numpy cast
 * is undefined, and here the value clamps to [0, 65535] (NaN: 0).  One launch.
 * SDF_E_NULL: d, flow or out NULL; SDF_E_SHAPE: as sdf_flow_image_fwd; SDF_E_ALIGN: flow not 4-byte or out not 2-byte aligned. */
typedef struct SdfFlowSubmissionDesc {
  const float* flow;
  void* out;
  int32_t B, H, W;
} SdfFlowSubmissionDesc;

int sdf_flow_submission_fwd(const SdfFlowSubmissionDesc* d, void* stream);

/* sdf_event_image_fwd: the loops' `chunk_vis` and the reference's events_to_image (green_red) of it, as the bytes cv2.imwrite stores.
 * stage 0: src -> chunk_vis (B, 2, h, w) fp32 on the window (crop_h, crop_w) at (crop_oy, crop_ox) (0, 0 at origin 0, 0: all of it).
 *   mode 0 (signed): src is a signed voxel (B, bins, Hs, Ws): pos = sum over bins of max(v, 0), neg = sum over bins of max(-v, 0)
 *                    (eval_DSEC_flow_SNN.py:182-188, eval_MV_flow_SNN.py:184)
 *   mode 1 (split):  src is the model's input (B, bins, 2, Hs, Ws): pos / neg = channel 0 / 1 summed over bins
 *   both added in bin order in fp32.
 * stage 1: chunk_vis and bounds (B, 4) fp32 = {pos_min, pos_max, neg_min, neg_max}, the 1st and 99th percentiles of each polarity of
 *   the sample (the caller's: any quantile routine on the stream) -> out (B, h, w, 3) u8.  In fp32: m = max(pos_max, neg_max);
 *   pos' = clip((pos - pos_min) / (m - pos_min), 0, 1) when pos_min != m, else clip(pos, 0, 1); neg' alike.  The reference's image is
 *   (0, pos', neg') and cv2.imwrite reads it as BGR, so the stored file's RGB is out = (neg', pos', 0), each byte rint(255 * x) in
 *   fp64 with halves to even: OpenCV's documented saturate_cast<uchar>(double) (taken from its documentation, not checked against cv2).
 * SDF_E_NULL: d, chunk_vis, src (stage 0), bounds or out (stage 1) NULL; SDF_E_DTYPE: mode or stage not 0 / 1; SDF_E_SHAPE: B, bins,
 * Hs or Ws < 1, B > 65535, a window outside the source, h w >= 2^30 or a source beyond 2^60 elements; SDF_E_ALIGN: a float pointer not
 * 4-byte aligned. */
typedef struct SdfEventImageDesc {
  const float* src;
  float* chunk_vis;
  const float* bounds;
  uint8_t* out;
  int32_t B, bins, Hs, Ws, crop_h, crop_w, crop_oy, crop_ox;
  int32_t mode, stage;
} SdfEventImageDesc;

int sdf_event_image_fwd(const SdfEventImageDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * fp32 membranes -> per-time-step statistics in integers: what a reader of the reference's `v_seq_monitor.records` (`vis.monitor_v`)
 * looks at - mean, extremes and a histogram of a neuron call's membrane per step - without keeping the membrane.
 * sdf_spike_count_fwd's geometry on fp32: element (o, t, r, c) is the float at v + ((o * T + t) * rows + r) * row_stride + c (strides
 * in elements).  Nothing outside the addressed floats is read: row_stride == C is one run of rows * C floats per (o, t), 16 bytes per
 * lane between the run's first and last 16-byte boundary and element-wise in front and behind; row_stride > C walks the rows.
 * Step t ADDS into the record table + t * (4 + bins + 2) of 64-bit integers:
 *   [0] n_nan    += NaNs (a NaN takes part in nothing else)
 *   [1] sum_q16  += (int64) rintf(clamp(x, -32768.f, 32768.f) * 65536.f)            (the product is exact in fp32)
 *   [2] min_key   = min(min_key, key(x)),  [3] max_key = max(max_key, key(x)),  key = bits ^ (sign ? 0xFFFFFFFF : 0x80000000), the
 *       order-preserving unsigned key of the fp32 bits; the CALLER initialises the slots to 2^32 - 1 and 0 (and the rest to 0)
 *   [4 + i] hist[i] += 1,  i = x < lo ? 0 : x >= hi ? bins + 1 : 1 + min(bins - 1, (int) floorf((x - lo) * inv_width)), every
 *       operation rounded separately; inv_width = bins / (hi - lo) is formed once by the caller in fp32
 * Integer atomics only: the same bits on every run, and restated exactly on the host (sdformerflow_amd/monitor.py membrane_record).
 * SDF_E_NULL: d, v or table NULL; SDF_E_SHAPE: outer, rows or C < 1, T outside 1 .. 64, row_stride < C, bins outside 1 .. 256, not
 * lo < hi, inv_width not positive and finite (or sizes beyond 2^60 elements / 2^31 workgroups); SDF_E_ALIGN: v not 4-byte or table not
 * 8-byte aligned.  Added to SDF_VERSION 107 (no existing entry changed). */
typedef struct SdfMembraneStatsDesc {
  const float* v;
  int64_t outer;
  int T;
  int64_t rows;
  int C;
  int64_t row_stride;
  int64_t* table;           /* T records of 4 + bins + 2 */
  int bins;
  float lo, hi, inv_width;
} SdfMembraneStatsDesc;

int sdf_membrane_stats_fwd(const SdfMembraneStatsDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The tail of a training step on flat fp32 gradient buckets (train.GradientBuckets): per-parameter gradient statistics (the
 * reference's `vis.store_grads`, utils/gradients.py), the clip coefficient of torch.nn.utils.clip_grad_norm_, and the AdamW update.
 * A parameter is a SEGMENT [offset, offset + length) of the flat buffer (in floats); segments are packed at any element offset, so
 * every kernel reads a segment's floats one by one in front of its first and behind its last 16-byte boundary and 16 bytes per lane
 * between them; nothing outside a segment is touched.  No host synchronisation and no float atomics anywhere.
 *
 * The segment tables are given TWICE, with the same contents: on the host (`*_host`: read by the entry point's checks before any
 * launch) and on the device (read by the kernels).  Checks shared by the three entry points, in this order: SDF_E_NULL: a required
 * pointer NULL; SDF_E_SHAPE: no segment or more than 65535, a buffer beyond 2^40 floats, an offset < 0, a length < 1, a segment that
 * starts in front of its predecessor's end (segments ascend and do not overlap) or ends behind the buffer, rows outside the table, a
 * workspace that is too small; SDF_E_ALIGN: a pointer not aligned as stated below; SDF_E_DTYPE: a pointer the kernels would
 * dereference is not device (or managed) memory as far as hipPointerGetAttributes can tell - a host pointer never reaches a launch.
 * Added to SDF_VERSION 107 (no existing entry changed).
 *
 * sdf_grad_stats_fwd: segment s of `flat` (n floats) writes row row0 + s of `table` (double[rows][5]; other rows are left alone):
 *   {sum_abs = sum |g|, sum_sq = sum g * g, min_abs, max_abs, nonfinite = #(inf, -inf, NaN)}
 * over the FINITE elements, |g| and g * g formed and added in fp64 (both exact), the count exact.  A segment without a finite element
 * has sum 0, min_abs +inf, max_abs 0.  Two launches: 128 workgroups per segment own fixed, interleaved 16 KiB chunks of it and write
 * one partial record each to the workspace (lane -> wave -> workgroup); a second kernel combines a segment's 128 partials in a fixed
 * order.  Two runs on the same bytes give the same bytes.
 * flat 4-byte aligned (any position within 16 bytes, the segments too), table / workspace 8-byte aligned, seg: int64[nseg][2] = {offset, length}.
 * workspace: sdf_grad_stats_workspace_bytes(nseg) bytes (0: refused nseg). */
typedef struct SdfGradStatsDesc {
  const float* flat;
  int64_t n;
  const int64_t* seg_host;
  const int64_t* seg;
  int32_t nseg, row0, rows;
  double* table;
  void* workspace;
  int64_t workspace_bytes;
} SdfGradStatsDesc;

int64_t sdf_grad_stats_workspace_bytes(int nseg);
int sdf_grad_stats_fwd(const SdfGradStatsDesc* d, void* stream);

/* sdf_grad_clip_coef: over the rows r of a sdf_grad_stats_fwd table (double[rows][5], every bucket's rows in one table) with
 * mask[r] != 0 (mask: rows bytes on the device, or NULL: every row), in fp64 and in a fixed order:
 *   total = sqrt(sum sum_sq[r]);   record[0] = total;   record[1] = sum nonfinite[r];
 *   coef[0] = (float) min(1, (double) max_norm / (total + 1e-6))
 * - clip_grad_norm_'s formula with the norm taken in fp64; max_norm +inf gives coef 1 (no clip).  One launch of one workgroup.
 * SDF_E_SHAPE: rows < 1 or > 2^24, max_norm NaN or < 0; table / record 8-byte, coef 4-byte aligned. */
int sdf_grad_clip_coef(const double* table, int rows, const uint8_t* mask, float max_norm, float* coef, double* record, void* stream);

/* sdf_adamw_step: torch.optim.AdamW(foreach=False)'s update of every ACTIVE segment, one read of g, m, v, p and one write of m, v, p.
 * Row s of `rows` names the parameter (its own fp32 storage, `length` contiguous floats), its segment of grad / exp_avg / exp_avg_sq
 * (three flat buffers of n floats with the same layout) and the step's scalars, rounded to fp32 as torch rounds the Python doubles:
 *   decay = 1 - lr * weight_decay, w1 = 1 - beta1, beta2, w2 = 1 - beta2, neg_step_size = -lr / (1 - beta1^step),
 *   bc2_sqrt = sqrt(1 - beta2^step), eps.
 * Per element, every operation rounded on its own in fp32, c = coef ? coef[0] : 1:
 *   g = grad * c;  p = p * decay;  m = w1 < 0.5 ? m + w1 * (g - m) : g - (g - m) * (1 - w1)  (torch's lerp);
 *   v = v * beta2;  v = v + (w2 * g) * g;  p = p + (neg_step_size * m) / (sqrt(v) / bc2_sqrt + eps)
 * grad itself is not written.  A row with active == 0 is not touched: not p, not the moments.  p is accessed 16 bytes per lane where it
 * shares the segment's position within 16 bytes, 4 bytes per lane otherwise.
 * grad / exp_avg / exp_avg_sq 4-byte aligned and at ONE position within 16 bytes, every param and coef 4-byte aligned, rows 8-byte
 * aligned; SDF_E_NULL also for a NULL param of an active row; SDF_E_DTYPE also for a param of an active row that is not device memory. */
typedef struct SdfAdamwRow {
  void* param;
  int64_t offset, length;
  float decay, w1, beta2, w2, neg_step_size, bc2_sqrt, eps;
  int32_t active;
} SdfAdamwRow;

typedef struct SdfAdamwDesc {
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t n;
  const SdfAdamwRow* rows_host;
  const SdfAdamwRow* rows;
  int32_t nseg;
  const float* coef;
} SdfAdamwDesc;

int sdf_adamw_step(const SdfAdamwDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same tail with a loss scaler (torch.amp.GradScaler's arithmetic), a skipped step and gradient accumulation: the decision "this
 * step is off" and the factor "multiply by this" live in device memory and the update obeys them; the host waits for neither.
 * Conventions, check order and alignment rules are those of the three entry points above.  Added to SDF_VERSION 107 (no existing
 * entry changed).
 *
 * SdfLossScaleState (device memory, 8-byte aligned): `scale` is what the NEXT loss is multiplied by; `inv_scale`, `found_inf` and
 * `skipped` are written by sdf_grad_clip_scale_coef: the reciprocal of the scale the gradients of THIS step carry, whether one of
 * them is not finite, and how many steps were found so since the state was made. */
typedef struct SdfLossScaleState {
  float scale;
  int32_t growth_tracker;
  float inv_scale;
  int32_t found_inf;
  int64_t skipped;
} SdfLossScaleState;

/* sdf_grad_scale_inplace: g = g * coef[0] over every segment s of `flat` with mask[s] != 0 (mask: nseg bytes on the device, or NULL:
 * every segment) - clip_grad_norm_'s in-place pass on a running sum, the coefficient read from device memory.  One fp32
 * multiplication per element (inf and NaN follow IEEE); 16 bytes per lane between a segment's 16-byte boundaries, single floats in
 * front of and behind them; one launch.  flat / coef 4-byte, seg 8-byte aligned; seg as in SdfGradStatsDesc. */
typedef struct SdfGradScaleDesc {
  float* flat;
  int64_t n;
  const int64_t* seg_host;
  const int64_t* seg;
  int32_t nseg;
  const uint8_t* mask;
  const float* coef;
} SdfGradScaleDesc;

int sdf_grad_scale_inplace(const SdfGradScaleDesc* d, void* stream);

/* sdf_grad_clip_scale_coef: sdf_grad_clip_coef's reduction (the same order, fp64) and, behind it in the same single workgroup, the
 * scaler.  With s0 = state->scale as it stands (the scale the gradients carry):
 *   total, record[0], record[1] as sdf_grad_clip_coef;   inv_scale = (float)(1.0 / (double) s0);
 *   coef[0] = (float) min(1, (double) max_norm / (t + 1e-6)),  t = clip_unscaled ? total * inv_scale : total
 *     (clip_unscaled 0: the clip bounds the STILL-SCALED norm, as a loop that calls clip_grad_norm_ without scaler.unscale_ does);
 *   found_inf = record[1] > 0;   skipped += found_inf;
 *   update != 0 - torch's _amp_update_scale_ on fp32 values:  found_inf: scale = s0 * backoff_factor, growth_tracker = 0;  else
 *     growth_tracker + 1 == growth_interval: scale = s0 * growth_factor unless that is not finite, growth_tracker = 0;  else
 *     growth_tracker += 1.   update == 0 leaves scale and growth_tracker alone (a scaler that only provides the skip).
 * SDF_E_SHAPE: rows < 1 or > 2^24, max_norm NaN or < 0, a factor that is NaN or <= 0, growth_interval < 1; table / record / state
 * 8-byte, coef 4-byte aligned. */
typedef struct SdfGradClipScaleDesc {
  const double* table;
  int32_t rows;
  const uint8_t* mask;
  float max_norm;
  float* coef;
  double* record;
  SdfLossScaleState* state;
  float growth_factor, backoff_factor;
  int32_t growth_interval, clip_unscaled, update;
} SdfGradClipScaleDesc;

int sdf_grad_clip_scale_coef(const SdfGradClipScaleDesc* d, void* stream);

/* sdf_adamw_step_scaled: sdf_adamw_step under a loss scaler.  state->found_inf != 0: no byte of a parameter or a moment is written by
 * any workgroup.  Otherwise sdf_adamw_step's arithmetic on g = (grad * c) * state->inv_scale - two fp32 multiplications, as
 * clip_grad_norm_'s in-place pass followed by GradScaler.unscale_ performs.  state: device memory, 8-byte aligned (SDF_E_NULL when NULL). */
int sdf_adamw_step_scaled(const SdfAdamwDesc* d, const SdfLossScaleState* state, void* stream);

/* ---------------------------------------------------------------------------------------------
 * u8 spikes -> spike counts per SAMPLE and time step: sdf_spike_count_fwd (below) generalised by the sample axis, for the records of
 * a replica forward (R independent batch-1 samples in one launch sequence), where one count per step would mix the samples.
 * Element (so, t, si, r, c) is the byte at spikes + ((((so * T + t) * s_in + si) * rows + r) * row_stride + c; the call computes
 *   counts[(so * s_in + si) * sample_pitch + t] += sum over r, c     (64-bit integers; the CALLER zeroes them)
 * for the s_out * s_in samples; sample_pitch (in int64 elements, >= T) lets the T counts of a sample lie inside a larger record, e.g. a
 * (samples, calls, Tmax) block with sample_pitch = calls * Tmax.  s_in = 1: the samples lie OUTSIDE time - channel-last
 * (B, D, h, w, C) activations and their channel slices.  s_out = 1: the samples are s_in equal consecutive pieces of every time block -
 * the (T', R * nW * N1, C) window records of a replica forward, the patch merging's (D, B, H2, W2, 4C), the halves of a stacked q | k
 * buffer (row_stride 2C).  Every (so, t, si) piece is a run of its own: row_stride == C reads 16 bytes per lane from the first
 * 16-byte boundary INSIDE the piece and the bytes in front of it and behind the last whole vector one by one, so nothing outside a
 * piece is read and no byte is added to a neighbouring sample; row_stride > C walks the rows (small tensors).  Integer sums, lane ->
 * wave -> workgroup, one 64-bit atomic per workgroup: the same bits on every run.  s_out = s_in = 1 equals sdf_spike_count_fwd with
 * outer 1.  Added to SDF_VERSION 107 (no existing entry changed).
 * SDF_E_NULL: d, spikes or counts NULL; SDF_E_SHAPE: s_out, s_in, rows or C < 1, T outside 1 .. 64, row_stride < C, sample_pitch < T
 * (or sizes beyond 2^62 bytes / 2^31 workgroups); SDF_E_ALIGN: counts not 8-byte aligned. */
typedef struct SdfSpikeCountSegDesc {
  const uint8_t* spikes;
  int64_t s_out;
  int T;
  int64_t s_in;
  int64_t rows;
  int C;
  int64_t row_stride;
  int64_t* counts;
  int64_t sample_pitch;
} SdfSpikeCountSegDesc;

int sdf_spike_count_seg_fwd(const SdfSpikeCountSegDesc* d, void* stream);

/* ---------------------------------------------------------------------------------------------
 * u8 spikes -> spike counts per time step: the numerator of the firing rate the reference's output monitor records for a neuron call,
 * `cal_firing_rate(s_seq) = s_seq.flatten(1).mean(1)` (eval_DSEC_flow_SNN.py:22-24, 140-143, `vis.monitor_fr`).
 * Element (o, t, r, c) is the byte at spikes + ((o * T + t) * rows + r) * row_stride + c; the call computes
 *   counts[t] += sum over o, r, c            (t = 0 .. T - 1; 64-bit integers; the CALLER zeroes them)
 * One addressing form for a contiguous (T, rows, C) tensor (outer 1), a channel-last (B, D, h, w, C) activation (outer B, T = D), a
 * channel slice [..., c0:c1] of a wider activation (row_stride = its channel count, spikes moved by c0 - any alignment) and the halves
 * of a stacked (M, 2C) q | k buffer (row_stride 2C).  Nothing outside the addressed bytes is read.  row_stride == C (one run of
 * rows * C bytes per (o, t)) is the fast path: 16 bytes per lane, byte-wise in front of the first and behind the last 16-byte
 * boundary; row_stride > C walks the rows and is meant for small tensors.  Sums are integers, added lane -> wave -> workgroup and then
 * with one 64-bit atomic per workgroup and step: the same bits on every run.  Added to SDF_VERSION 107 (no existing entry changed).
 * SDF_E_NULL: d, spikes or counts NULL; SDF_E_SHAPE: outer, rows or C < 1, T outside 1 .. 64, row_stride < C (or sizes beyond 2^62
 * bytes / 2^31 workgroups); SDF_E_ALIGN: counts not 8-byte aligned. */
typedef struct SdfSpikeCountDesc {
  const uint8_t* spikes;
  int64_t outer;
  int T;
  int64_t rows;
  int C;
  int64_t row_stride;
  int64_t* counts;
} SdfSpikeCountDesc;

int sdf_spike_count_fwd(const SdfSpikeCountDesc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDFORMERFLOW_HIP_H */
