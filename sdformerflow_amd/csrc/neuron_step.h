// One time step of a spiking neuron (charge, fire, reset) and one step of its backward through time: the only place in csrc/ where
// they are written.  Every operation is a separately rounded fp32 op in the reference's order (spikingjelly's LIFNode / IFNode /
// ParametricLIFNode under torch autograd; the files that include this are compiled with -ffp-contract=off), which is what the
// bit-for-bit tests against oracle/ and tests/golden/ pin.  All flags are wave-uniform.
//
// Deliberate restatements of lif_step_fast (same value, the reset as a select on the comparison's own difference, inside the
// kernels whose epilogue's vector instructions bound them): spike_mm.h neuron_T<0>, head_tail.hip `if constexpr (fast)`,
// spike_conv_wres.hip `if (lif_fast)`.
// Sites that keep neuron_charge + fire_reset written out, because calling them changed a register count of a kernel that
// inlines the site (tools/kernel_resources.py): the generic branch of spike_mm.h lif_steps (ms_wide.hip wide_pm_kernel at T = 20)
// and the generic branch of head_tail.hip head_conv_mfma_kernel.  A change to the sequence below is made there too.
// For the same reason neuron.hip plif_fwd_kernel charges through lif_charge(tau = inf, inv_tau = k), not plif_charge.
#pragma once

__device__ __forceinline__ float if_charge(float v, float x) { return v + x; }

// x - (v - v_reset); reset0 = (soft reset or v_reset == 0) takes the subtraction of zero out
__device__ __forceinline__ float charge_diff(float v, float x, float v_reset, bool reset0) {
  return reset0 ? (x - v) : (x - (v - v_reset));
}

__device__ __forceinline__ float lif_charge(float v, float x, float tau, float inv_tau, float v_reset, bool reset0) {
  float d = charge_diff(v, x, v_reset, reset0);
  float q = (inv_tau != 0.f) ? d * inv_tau : d / tau;   // power-of-two tau: multiplication is exact
  return v + q;
}

__device__ __forceinline__ float neuron_charge(bool is_if, float v, float x, float tau, float inv_tau, float v_reset, bool reset0) {
  return is_if ? if_charge(v, x) : lif_charge(v, x, tau, inv_tau, v_reset, reset0);
}

// PLIF: the multiplier k = sigmoid(w) in place of 1 / tau; d is the charge difference dL/dk needs
__device__ __forceinline__ float plif_charge(float v, float x, float k, float v_reset, bool reset0, float& d) {
  d = charge_diff(v, x, v_reset, reset0);
  return v + d * k;
}

__device__ __forceinline__ float spike_of(float h, float v_th) { return (h - v_th >= 0.f) ? 1.f : 0.f; }

__device__ __forceinline__ float fire_reset(float& v, float h, float v_th, float v_reset, bool soft) {
  float s = spike_of(h, v_th);
  v = soft ? (h - s * v_th) : ((1.f - s) * h + s * v_reset);
  return s;
}

// the shipped configuration - LIF, soft reset, tau a power of two - as a branch-free step
__device__ __forceinline__ float lif_step_fast(float& v, float x, float inv_tau, float v_th) {
  const float h = v + (x - v) * inv_tau;
  const float s = spike_of(h, v_th);
  v = h - s * v_th;
  return s;
}

// ATan surrogate, torch: alpha / 2 / (1 + (pi / 2 * alpha * u).pow(2)) * g   ==   ((1 + t*t).reciprocal() * (alpha/2)) * g
// c = (float)(pi/2 * alpha), ha = (float)(alpha/2): sdf_atan_consts (common.h)
__device__ __forceinline__ float sg_atan(float u, float g, float c, float ha) {
  const float t = c * u;
  const float y = 1.f + t * t;
  return ((1.f / y) * ha) * g;
}

// dL/dh_t from gv = dL/dv_t (flowing back from step t+1) and gs = dL/ds_t; the reset path joins gs unless it is detached
__device__ __forceinline__ float bptt_gh(float gv, float gs, float h, float s, float v_th, float v_reset, bool soft, bool detach,
                                         float c, float ha) {
  const float u = h - v_th;
  if (soft) {                                                  // v_t = h - s * v_th
    if (!detach) gs = gs + (-(gv * v_th));
    return gv + sg_atan(u, gs, c, ha);
  }
  if (!detach) gs = gs + (gv * v_reset + (-(gv * h)));         // v_t = (1 - s) * h + s * v_reset
  return gv * (1.f - s) + sg_atan(u, gs, c, ha);
}

// dL/dx_t and dL/dv_{t-1} from gh, per charge form (v_reset is a constant)
__device__ __forceinline__ void neuron_charge_bwd(bool is_if, float gh, float tau, float inv_tau, float& gx, float& gv) {
  if (is_if) {                                                 // h = v + x
    gx = gh;
    gv = gh;
    return;
  }
  const float qd = (inv_tau != 0.f) ? gh * inv_tau : gh / tau; // h = v + (x - v) / tau
  gx = qd;
  gv = gh - qd;
}
__device__ __forceinline__ void plif_charge_bwd(float gh, float k, float& gx, float& gv) {
  const float qd = gh * k;
  gx = qd;
  gv = gh - qd;
}

// GLIF (the reference's GatedLIFNode with layer-wise gates, Spiking_submodules.py:152-180).  The host forms the derived gates once:
// L = 1 - a (1 - sigmoid(tau)), Dk = (1 - a) sigmoid(linear_decay), g = sigmoid(gamma), R = (1 - g) sigmoid(v_subreset),
// th = sigmoid(v_threshold), and per step c_t = 1 - b (1 - sigmoid(conduct_t)), a = sigmoid(alpha), b = sigmoid(beta).
struct GlifGates { float L, Dk, g, R, th; };

// one step: charge with the previous membrane v and spike s, reset by s, fire; v becomes u (the spike is NOT subtracted from v:
// the reset of step t acts inside step t + 1).  Returns u_t.
__device__ __forceinline__ float glif_step(float& v, float& s, float x, float c, const GlifGates& G) {
  const float inp = x * c;
  const float lv = G.L * v;
  float u = (lv - G.Dk) + inp;
  u = (u - (lv * G.g) * s) - G.R * s;
  s = spike_of(u, G.th);
  v = u;
  return u;
}

// one step of its backward: gu = dL/du_{t+1} on entry, dL/du_t on return; u, s = u_t, s_t; gs = dL/ds_t.  sg = the surrogate term
// (dL/dth sums its negative).  The spike is not detached: dL/ds_t takes the reset path of step t + 1.
__device__ __forceinline__ float glif_bwd_step(float gu, float gs, float u, float s, const GlifGates& G, float c_atan, float ha, float& sg) {
  const float S = gs + gu * (-((G.L * u) * G.g) - G.R);
  const float V = gu * (G.L - (G.L * G.g) * s);
  sg = sg_atan(u - G.th, S, c_atan, ha);
  return V + sg;
}
