// step_trunc.h — the episode-length truncation test as an integer compare
// (plain C++, no HIP).
//
// The reference truncates an episode when step_counter / PYB_FREQ >
// EPISODE_LEN_SEC (MultiHoverAviary.py:267-268), a double division of the
// integer counter by the integer frequency.  IEEE division is correctly rounded
// and the quotient does not decrease when the counter grows, so the test is true
// exactly for the counters from some smallest one upwards.  qs_create finds that
// counter once per handle (trunc_threshold) and the step kernel compares its
// counter against it instead of dividing in every step.
#pragma once

#include <cstdint>

namespace qs {

// The division form, as the reference and the oracle evaluate it.
inline bool trunc_by_division(int64_t n, int pyb_freq, double ep_len_sec) {
  return ((double)n / (double)pyb_freq) > ep_len_sec;
}

constexpr int64_t kTruncNever = INT64_MAX;

// The smallest n >= 0 with (double)n / (double)pyb_freq > ep_len_sec, found by
// evaluating exactly that expression around floor(ep_len_sec · pyb_freq).
// kTruncNever: no n below 2^53 (every such n is an exact double) satisfies it
// — a NaN or an episode length no counter can reach.
inline int64_t trunc_threshold_exact(int pyb_freq, double ep_len_sec) {
  if (pyb_freq <= 0 || ep_len_sec != ep_len_sec) return kTruncNever;
  const double guess = ep_len_sec * (double)pyb_freq;
  if (!(guess < 9007199254740992.0 - 8.0)) return kTruncNever;   // 2^53
  int64_t n = guess > 2.0 ? (int64_t)guess - 2 : 0;   // the product is off by an ulp at most
  while (n > 0 && trunc_by_division(n - 1, pyb_freq, ep_len_sec)) --n;
  while (!trunc_by_division(n, pyb_freq, ep_len_sec)) ++n;
  return n;
}

// The same, clamped to INT32_MAX when no int32 counter reaches it (the step
// kernel's Params::trunc_at; the kernel tests step_counter >= trunc_at).
inline int32_t trunc_threshold(int pyb_freq, double ep_len_sec) {
  const int64_t n = trunc_threshold_exact(pyb_freq, ep_len_sec);
  return n > (int64_t)INT32_MAX ? INT32_MAX : (int32_t)n;
}

}  // namespace qs
