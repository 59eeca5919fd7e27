// Host side shared by the stand-alone neuron entry points (neuron.hip, neuron_bwd.hip, glif.hip, qk_gate_train.hip): the T values
// their kernels are instantiated for, the dispatch from a runtime T to one instantiation, and the grid of the streaming shape.
// Host code only - the device side of the family is neuron_step.h / device_prims.h.
#pragma once
#include <stdint.h>
#include <type_traits>

template <int... Ts>
struct SdfTList {};

// Each legal set of T is written here and nowhere else.
inline constexpr SdfTList<1, 2, 4, 5, 8, 10, 16, 20> SDF_T_STREAM{};   // streaming neuron kernels (T loads in flight per lane)
inline constexpr SdfTList<2, 4, 5, 10, 20> SDF_T_GLIF{};               // GLIF forward / backward and the multi-descriptor forward
inline constexpr SdfTList<1, 2, 4> SDF_T_GATE{};                       // T' attention steps of the training token gate

template <int... Ts>
static inline bool sdf_T_in(SdfTList<Ts...>, int T) {
  return ((T == Ts) || ...);
}

// Calls f(std::integral_constant<int, TT>{}) for the TT of the list equal to T; false when T is not in the list (f is not called).
// The SDF_LAUNCH of kernel<tt, ...> stays in f at the call site, so the launch log sees the kernel's own function pointer.
// (Head-first recursion with f named before the tail, not a fold: the compiler then emits the kernels in the order of the list.)
template <class F>
static inline bool sdf_for_T(SdfTList<>, int, F&&) {
  return false;
}
template <int T0, int... Ts, class F>
static inline bool sdf_for_T(SdfTList<T0, Ts...>, int T, F&& f) {
  if (T == T0) {
    f(std::integral_constant<int, T0>{});
    return true;
  }
  return sdf_for_T(SdfTList<Ts...>{}, T, f);
}

// Workgroups of the streaming shape - 4 consecutive neurons per lane, 256 lanes per workgroup - over n neurons.  Every launch of
// that shape and every *_workspace_bytes that holds one row of partials per workgroup takes its count from here.
static inline int64_t sdf_quad_blocks(int64_t n) { return (n / 4 + 255) / 256; }
