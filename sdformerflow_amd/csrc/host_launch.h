// Host side shared by the entry points: the dispatch from a runtime value to one template instantiation over a stated list (the only
// place a ladder over several values is written; a two-way `if` over one boolean stays an `if`), the launch-error tail, the neuron-configuration check, the neuron
// classes, the T values of the stand-alone neuron kernels (neuron.hip, neuron_bwd.hip, glif.hip, qk_gate_train.hip) and the grid of
// their streaming shape.  The digit-plane product kernels' own host rules are in digit_host.h.
// Host code only - the device side of the neuron family is neuron_step.h / device_prims.h.
#pragma once
#include "common.h"
#include <type_traits>

template <int... Vs>
struct SdfList {};

// The legal T sets of the neuron entry points are written here and nowhere else; a kernel family with a set of its own (T, neuron
// class, column blocks, a boolean as <0, 1>) writes it at the dispatch, where `if constexpr` leaves out the combinations it has no
// kernel for.
inline constexpr SdfList<1, 2, 4, 5, 8, 10, 16, 20> SDF_T_STREAM{};   // streaming neuron kernels (T loads in flight per lane)
inline constexpr SdfList<2, 4, 5, 10, 20> SDF_T_GLIF{};               // GLIF forward / backward and the multi-descriptor forward
inline constexpr SdfList<1, 2, 4> SDF_T_GATE{};                       // T' attention steps of the training token gate

// Compile-time classes of a neuron setting (spike_mm.h neuron_class): 0 = LIF with a soft reset and an exact 1 / tau, 1 = PSN,
// 2 = the general LIF / IF step.  Class 1 keeps its T x T coefficients in registers or an LDS table and is built for
// T <= 10 only, and every launch function that instantiates a <T, class> pair asks here.
inline constexpr SdfList<0, 1, 2> SDF_NEURON_CLASSES{};
constexpr bool sdf_class_has_T(int nk, int T) { return nk != 1 || T <= 10; }

template <int... Vs>
constexpr bool sdf_in(SdfList<Vs...>, int v) {
  return ((v == Vs) || ...);
}

// Calls f(std::integral_constant<int, V>{}) for the V of the list equal to v; false when v is not in the list (f is not called).
// The SDF_LAUNCH of kernel<V, ...> stays in f at the call site, so the launch log sees the kernel's own function pointer; several
// runtime values nest.  (Head-first recursion with f named before the tail, not a fold: the compiler then emits the kernels in the
// order of the list.)
template <class F>
static inline bool sdf_dispatch(SdfList<>, int, F&&) {
  return false;
}
template <int V0, int... Vs, class F>
static inline bool sdf_dispatch(SdfList<V0, Vs...>, int v, F&& f) {
  if (v == V0) {
    f(std::integral_constant<int, V0>{});
    return true;
  }
  return sdf_dispatch(SdfList<Vs...>{}, v, f);
}

// What a launch function returns behind its last SDF_LAUNCH: 0 or the hipError_t of the launch (SDF_LAUNCH_CHECK as a value).
static inline int sdf_launch_rc() {
  const hipError_t e = hipGetLastError();
  return e != hipSuccess ? (int)e : 0;
}

// The neuron configuration an entry point accepts, as a value: SDF_E_DTYPE for a kind that is not LIF / PSN / IF, then SDF_E_NULL for
// PSN without both of its pointers, then SDF_E_SHAPE for a LIF tau the charge step has no form for (common.h sdf_tau_ok); else 0.
// The entry points call it where their own three clauses stood, so its place among their other checks is unchanged.  Two families
// keep their own, because other checks stand BETWEEN the clauses or the rule differs: neuron.hip (`validate`: the kind, then strides
// and alignment, then the PSN pointers; `launch_scalar` has no kind clause) and qk_gate_train.hip (the PSN pointers before the
// alignment, the kind behind the shape in `fill`, and no multiplicative tau < 1).  ms_wide.hip / ms_smallm.hip accept LIF / IF only:
// another rule.
static inline int sdf_neuron_cfg_rc(int kind, float tau, const float* psn_w, const float* psn_b) {
  if (kind != SDF_LIF && kind != SDF_PSN && kind != SDF_IF) return SDF_E_DTYPE;
  if (kind == SDF_PSN && (!psn_w || !psn_b)) return SDF_E_NULL;
  if (!sdf_tau_ok(kind, tau)) return SDF_E_SHAPE;
  return 0;
}
static inline int sdf_neuron_cfg_rc(const SdfNeuronCfg& n) { return sdf_neuron_cfg_rc(n.kind, n.tau, n.psn_w, n.psn_b); }

// Workgroups of the streaming shape - 4 consecutive neurons per lane, 256 lanes per workgroup - over n neurons.  Every launch of
// that shape and every *_workspace_bytes that holds one row of partials per workgroup takes its count from here.
static inline int64_t sdf_quad_blocks(int64_t n) { return (n / 4 + 255) / 256; }
