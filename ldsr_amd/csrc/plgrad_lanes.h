// plgrad_lanes.h -- the cross-lane part of the one-wave-per-cell time recursions: inclusive scans of plgrad.h's
// maps over the 64 lanes of a wavefront by DPP row shifts and broadcasts (no LDS), the value of the lane below
// and the fence between two passes over a wave's strip.  Shared by plgrad.hip (the penalised likelihood, its
// gradient, the L-BFGS learner on it) and filter.hip (the Kalman filter's outputs).  Device code only.
#pragma once
#include "plgrad.h"
#include "em_scan_impl.h"     // dppd, readlane_d, wave_sum_n

#pragma clang fp contract(off)

template <int CTRL, int RM>
__device__ __forceinline__ PlgAff aff_from(const PlgAff &x) {       // identity where the DPP source does not exist
    return PlgAff{dppd<CTRL, RM>(1.0, x.a), dppd<CTRL, RM>(0.0, x.b)};
}
// inclusive scan over the lanes: lane l gets (map of lane l) after ... after (map of lane 0)
__device__ __forceinline__ PlgAff aff_scan(PlgAff x) {
    x = plg_aff_then(aff_from<DPP_ROW_SHR(1), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_SHR(2), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_SHR(4), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_SHR(8), 0xF>(x), x);
    x = plg_aff_then(aff_from<DPP_ROW_BCAST15, 0xA>(x), x);          // lane 15 -> row 1, lane 47 -> row 3
    x = plg_aff_then(aff_from<DPP_ROW_BCAST31, 0xC>(x), x);          // lane 31 -> rows 2, 3
    return x;
}

template <int CTRL, int RM>
__device__ __forceinline__ PlgMob mob_from(const PlgMob &x) {
    return PlgMob{dppd<CTRL, RM>(1.0, x.m00), dppd<CTRL, RM>(0.0, x.m01), dppd<CTRL, RM>(0.0, x.m10),
                  dppd<CTRL, RM>(1.0, x.m11)};
}
__device__ __forceinline__ PlgMob mob_scan(PlgMob x) {
    x = plg_mob_then(mob_from<DPP_ROW_SHR(1), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_SHR(2), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_SHR(4), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_SHR(8), 0xF>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_BCAST15, 0xA>(x), x);
    x = plg_mob_then(mob_from<DPP_ROW_BCAST31, 0xC>(x), x);
    return x;
}

// the value of the lane below (the step before in a forward pass, the step above in a backward one); lane 0
// gets the carry of the chunk before
__device__ __forceinline__ double lane_below(double carry, double x) { return dppd<DPP_WAVE_SHR1, 0xF>(carry, x); }

// a wave's strip is written by one lane and read by another in the next pass
__device__ __forceinline__ void strip_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
