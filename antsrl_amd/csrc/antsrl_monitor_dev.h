// antsrl_monitor_dev.h — the device side of THE ORDER OF THE SUMS (antsrl_monitor.h), shared by the monitor's kernels
// (antsrl_monitor.hip) and the population's fitness (antsrl_popfitness.hip): what one of the 256 slots does with an
// element, and the folds of the slots.  Every add is a float64 add; the build's -ffp-contract=off keeps it one.
#pragma once
#include <hip/hip_runtime.h>
#include "antsrl_monitor.h"

// slot t takes element v (the i-th of the row, i = t, t + 256, ... ascending): the sum, and min / max from the slot's
// first element on
__device__ __forceinline__ void monitor_slot_take(double v, bool first, double &sum, double &mn, double &mx)
{
    sum = sum + v;
    mn = (first || v < mn) ? v : mn;
    mx = (first || v > mx) ? v : mx;
}

// x[i] += x[i + s] for i < s, s = 128, ..., 1, over the workgroup's 256 slots; the result in x[0]
__device__ __forceinline__ void monitor_fold(double *x, int t)
{
    __syncthreads();
    for (int s = MON_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) x[t] = x[t] + x[t + s];
        __syncthreads();
    }
}

// monitor_fold of xs with the min and max of the slots that hold an element: a row of n elements fills slots [0, n)
// (the slots with one are a prefix, before and after every fold); the results in xs[0], xmn[0], xmx[0]
__device__ __forceinline__ void monitor_fold3(double *xs, double *xmn, double *xmx, int t, int n)
{
    __syncthreads();
    for (int s = MON_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            xs[t] = xs[t] + xs[t + s];
            if (t + s < n) {
                xmn[t] = xmn[t + s] < xmn[t] ? xmn[t + s] : xmn[t];
                xmx[t] = xmx[t + s] > xmx[t] ? xmx[t + s] : xmx[t];
            }
        }
        __syncthreads();
    }
}

// total[e] of antsrl_monitor.h for the row er[0 .. N): the slots' sums in xs, folded; every lane returns xs[0].  The
// caller separates two calls on the same xs with a __syncthreads().
__device__ __forceinline__ double monitor_row_total(const double *er, int N, double *xs, int t)
{
    double sum = 0.0;
    for (int n = t; n < N; n += MON_THREADS) sum = sum + er[n];
    xs[t] = sum;
    monitor_fold(xs, t);
    return xs[0];
}
