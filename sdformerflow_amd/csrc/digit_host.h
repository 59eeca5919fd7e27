// Host side shared by the int8 digit-plane product kernels (ms_res.hip, ms_wide.hip, ms_smallm.hip, spike_conv_wres.hip and their
// entry points in spike_gemm.hip): each grid rule, shape predicate and parameter filler of the family is stated here once.
// Host code only - the device side is wide_common.h / device_prims.h / neuron_step.h.
#pragma once
#include "wide_common.h"
#include "switches.h"
#include "host_launch.h"
#include <stdlib.h>

namespace sdfmm {

// ---- grids -----------------------------------------------------------------------------------------------------------------
// Units of the position-major kernels: a wave owns 80 rows = 4 * (20 / T) positions x T steps.
static inline int64_t pm_units(int64_t positions, int T) {
  const int ppw = 4 * (20 / T);
  return (positions + ppw - 1) / ppw;
}

// One workgroup per work item, rounded up to a multiple of 8 (the kernels deal the items round-robin over the 8 XCDs and let the
// surplus workgroups return).  `bounded`: refuse item counts the 32-bit grid cannot hold - the sites that passed no such check before
// this rule was stated once (launch_wide_merge, launch_wide_conv, launch_smallm_conv: their row limits keep them far below) still pass none.
static inline int grid8(int64_t items, dim3& grid, bool bounded = true) {
  if (bounded && items >= (1LL << 31) - 8) return SDF_E_SHAPE;
  grid = dim3((unsigned)((items + 7) / 8 * 8));
  return 0;
}

// K-ring position-major kernel (ms_wide.hip) with `cb` column blocks per wave: fills nunits / nrg / ncg / passes and sizes the grid.
// One workgroup per compute unit (the kernels take most of its registers): a launch of up to four rounds runs as ONE round of
// workgroups that walk several row groups (the prologue is paid once, no second dispatch wave).  `tuned` = the products of a block
// (SDF_WIDE_PASSES applies, the item count is bounded); patch merging passes false and keeps neither.
static inline int pm_ring_grid(WidePmParams& P, int T, int cb, bool tuned, dim3& grid) {
  const int64_t units = pm_units(P.P, T);
  if (!cb || units >= (1LL << 28)) return SDF_E_SHAPE;
  P.nunits = (int)units;
  P.nrg = (int)((units + 3) / 4);
  P.ncg = P.N / (16 * cb);
  const int64_t all = (int64_t)P.ncg * P.nrg;
  P.passes = all > 256 && all <= 1024 ? (int)((all + 255) / 256) : 1;
  if (tuned)
    if (const char* e = sdf_sw(SW_WIDE_PASSES)) { const int v = atoi(e); if (v >= 1 && v <= 8) P.passes = v; }     // tuning override
  return grid8((int64_t)P.ncg * ((P.nrg + P.passes - 1) / P.passes), grid, tuned);
}

// Weight-resident row-loop kernels (ms_res.hip): one workgroup per compute unit, all resident in one round - the smallest number r of
// units per wave for which (column groups) x (row ranges of 8 r units) fits the chip's 256 compute units.  Returns the row ranges of
// `n` units beside `cols` column groups, `per` = units per range.
static inline int64_t res_row_ranges(int64_t cols, int64_t n, int& per) {
  int r = 1;
  while (cols * ((n + 8 * r - 1) / (8 * r)) > 256) ++r;
  if (const char* e = sdf_sw(SW_RES_UPW)) { const int v = atoi(e); if (v >= 1 && v <= 4096) r = v; }     // tuning override: units per wave
  if (const char* e = sdf_sw(SW_RES_RMUL)) { const int v = atoi(e); if (v >= 1 && v <= 16) r *= v; }       // tuning: fewer, longer-lived workgroups
  per = 8 * r;
  return (n + per - 1) / per;
}

// ---- shapes ----------------------------------------------------------------------------------------------------------------
// the nine taps of a 3x3 kernel with padding 1 over K = 9 Cin in (tap, channel) order ...
static inline bool conv_taps_3x3_p1(const ConvGeom& cv, int K) {
  return cv.KWc == 3 && K == 9 * cv.Cin && cv.dy[0] == -1 && cv.dy[1] == 0 && cv.dy[2] == 1 && cv.dx[0] == -1 && cv.dx[1] == 0 && cv.dx[2] == 1;
}
// ... at stride 1: the output is the input's size
static inline bool conv_3x3_s1_p1(const ConvGeom& cv, int K) {
  return conv_taps_3x3_p1(cv, K) && cv.sy == 1 && cv.sx == 1 && cv.OH == cv.H && cv.OW == cv.W;
}

// T of a convolution whose rows are (b, t, pixel): the fused neuron's, else inferred from the image count; 0 = neither 10 nor 20 fits
static inline int conv_T(const SdfSpikeGemmDesc& d, int64_t imgs) {
  return d.sn_T ? d.sn_T : (imgs % 10 == 0 ? 10 : (imgs % 20 == 0 ? 20 : 0));
}

// the neuron of a GEMM descriptor; without_psn: for kernels that have no PSN epilogue (their class is then never 1)
static inline SdfNeuronCfg gemm_neuron(const SdfSpikeGemmDesc& d, bool with_psn = true) {
  return {d.sn_kind, d.tau, d.v_th, d.v_reset, d.soft_reset, with_psn ? d.psn_w : nullptr, with_psn ? d.psn_b : nullptr};
}

// ---- WidePmParams of the entry points that are one product ---------------------------------------------------------------------
// plain rows x digit planes with the fp32 epilogue: rows are walked as 10 "steps" x M / 10 "positions" (any order serves that form);
// the shortcut, if any, is the output buffer itself
static inline WidePmParams pm_plain(const SdfSpikeGemmDesc* d) {
  WidePmParams P = {};
  P.A = d->A; P.W = reinterpret_cast<const int8_t*>(d->Wp); P.cscale = d->col_scale; P.N = d->N; P.K = d->K;
  P.HW = (int)(d->M / 10); P.P = d->M / 10;
  P.bias = d->bias; P.alpha = d->alpha; P.beta = d->beta; P.x = d->out; P.ldo = (int)d->ldo; P.no_resid = d->resid ? 0 : 1;
  return P;
}
// patch merging: out = BN( [2x2 concat of the spikes] W^T ), a new tensor
static inline WidePmParams pm_merge(const SdfMsMergeDesc* d) {
  WidePmParams P = {};
  P.A = d->spikes; P.W = d->digits; P.cscale = d->cscale; P.N = d->N; P.K = 4 * d->C;
  P.HW = ((d->H + 1) / 2) * ((d->W + 1) / 2); P.P = (int64_t)d->B * P.HW;
  P.alpha = d->alpha; P.beta = d->beta; P.x = d->out; P.ldo = d->N; P.no_resid = 1;
  P.cv_H = d->H; P.cv_W = d->W; P.cv_Cin = d->C; P.cv_cpt = d->C / 64;          // (64-deep steps per quadrant)
  return P;
}
// stride-2 3x3 transposed convolution as one product over the 2 x 2 input neighbourhood (ms_res.hip, AM = 3)
static inline WidePmParams pm_deconv2x2(const SdfSpikeDeconvDesc* d) {
  WidePmParams P = {};
  P.A = d->spikes; P.W = d->digits; P.cscale = d->cscale; P.N = 4 * d->Cout; P.K = 4 * d->Cin;
  P.HW = d->H * d->W; P.P = (int64_t)(d->imgs / d->T) * P.HW;
  P.alpha = d->alpha; P.beta = d->beta; P.x = d->out; P.ldo = d->Cout; P.no_resid = 1;
  P.cv_H = d->H; P.cv_W = d->W; P.cv_Cin = d->Cin; P.dc_cout = d->Cout;
  return P;
}

}  // namespace sdfmm
