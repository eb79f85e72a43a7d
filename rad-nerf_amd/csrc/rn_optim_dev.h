// rn_optim_dev.h -- the arithmetic the reference's training loop wraps around its optimizer, plain functions for host and device:
// the learning-rate schedule (main.py:219: LambdaLR, 0.1 ** (iter / iters), 0.05 with --finetune_lips) and the decay of the weight
// average (torch_ema.ExponentialMovingAverage.update with use_num_updates).  No HIP header is needed: a host compiler builds the
// same text (tests/test_train_sched_abi.py does), k_adam_begin_sched of rn_train.hip includes it as it is.
//
// Both run ONCE per step, in one thread, in double; what the update kernel reads are the two floats they return.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef RN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define RN_HD __host__ __device__ inline
#else
#define RN_HD inline
#endif
#endif

namespace rn {
namespace optim {

// The rate of step s (counted from 1): LambdaLR has taken s - 1 steps when Trainer.train_one_epoch reaches optimizer.step() for
// the s-th time (nerf/utils.py:1030-1034).  gamma == 1 is a constant rate whatever iters is.
RN_HD float sched_lr(float lr0, double gamma, int32_t s, uint32_t iters) {
    if (gamma == 1.0) return lr0;
    return (float)((double)lr0 * pow(gamma, (double)(s - 1) / (double)iters));
}

// 1 - decay of the update that brings the count to num_updates: the warm-up (1 + n) / (10 + n) until it passes `decay`
// (n = 171 for 0.95), the constant afterwards.
RN_HD float ema_one_minus_decay(double decay, int32_t num_updates) {
    const double n = (double)num_updates;
    const double warm = (1.0 + n) / (10.0 + n);
    return (float)(1.0 - (decay < warm ? decay : warm));
}

// torch_ema's update of one element: tmp = shadow - param; tmp *= one_minus_decay; shadow -= tmp.  Three fp32 operations, each
// rounded on its own (the tree builds with -ffp-contract=off).
RN_HD float ema_one(float shadow, float param, float one_minus_decay) {
    float tmp = shadow - param;
    tmp = tmp * one_minus_decay;
    return shadow - tmp;
}

}  // namespace optim
}  // namespace rn
