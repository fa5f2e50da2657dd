// static_dispatch.h - a runtime value the caller has already checked, handed to
// a generic lambda as a compile-time constant: the one place a launcher writes
// its "H == 5 / else" or "learnt plant / analytic plant" ladder.
//   with_horizon(H, [&](auto h) { hipLaunchKernelGGL(kernel<h()>, ...); });
// Host only; shared by the shooting-MPC launchers of quad_mpc.hip and
// cartpole_mpc.hip.
#pragma once
#include <type_traits>

namespace apg {
namespace {

// H in {5, 10} (the caller's argument rule) -> std::integral_constant<int, H>
template <class F>
inline void with_horizon(int H, F &&f) {
  if (H == 5) f(std::integral_constant<int, 5>{});
  else f(std::integral_constant<int, 10>{});
}

template <class F>
inline void with_flag(bool on, F &&f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace
}  // namespace apg
