// csrc/sepaihrd_bitonic.inc -- the bitonic network of the segment sorts, device only: one text for the sort-and-pick
// kernels of csrc/sepaihrd_segment_sort.inc and for states_sort_pick_kernel of csrc/sepaihrd_particle_states.hip.
#pragma once

namespace sepaihrd {

// The Np (a power of two) doubles of seg sorted ascending in place by the whole workgroup.  The caller has stored the values
// and passed a barrier.  seg is LDS or, beyond what LDS holds, the segment itself in device memory: a barrier ends every round
// and makes a wave's stores visible to the workgroup (as in wide_resample_kernel), and no other workgroup touches the segment,
// so the barrier suffices there too.
__device__ __forceinline__ void bitonic_sort_pow2(double* seg, const int Np) {
    const int tid = threadIdx.x, BS = blockDim.x;
    for (int k = 2; k <= Np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (Np >> 1); i += BS) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));  // index with bit j clear
                const int hi = lo | j;
                const bool up = (lo & k) == 0;
                const double x = seg[lo], y = seg[hi];
                if ((x > y) == up) { seg[lo] = y; seg[hi] = x; }
            }
            __syncthreads();
        }
    }
}

// Np (a power of two) doubles of src sorted ascending into seg (LDS) by the whole workgroup
__device__ __forceinline__ void lds_bitonic_sort(double* seg, const double* src, const int Np) {
    const int tid = threadIdx.x, BS = blockDim.x;
    for (int i = tid; i < Np; i += BS) seg[i] = src[i];
    __syncthreads();
    bitonic_sort_pow2(seg, Np);
}

}  // namespace sepaihrd
