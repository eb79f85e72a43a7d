// rn_freq_dev.h -- one frequency of the frequency encoding as the torso kernels spell it: freq(x, deg) =
// [x, sin(2^f x), cos(2^f x)]_f with the cosine as a shifted sine.  The inference pass (k_torso_fused), the training
// forward (k_train_torso_fwd), the pose encoding (rn_torso_dev.h) and the FREQ operand of the weight gradients
// (rn_wgrad_dev.h) must agree to the bit: the weight gradients recompute enc_x and do not read a saved copy.
#pragma once

#include "rn_common.h"

namespace rn {

constexpr float kHalfPi = 3.141592653589793f / 2;

// angle 2^f x of frequency f, and its two features
__device__ __forceinline__ float freq_angle(float x, int f) { return scalbnf(x, f); }
__device__ __forceinline__ float freq_sin(float a) { return sinf(a); }
__device__ __forceinline__ float freq_cos(float a) { return sinf(a + kHalfPi); }

}  // namespace rn
