// schedule.hip -- difficulty-ordered team placement for launches with more waves than SIMDs.
//
// The team kernel's time is the busiest SIMD's: a wave iterates until its slowest team converges, and when
// a SIMD holds two or more waves they share its issue slots. A robot's IPM iteration count persists from
// tick to tick (DESIGN.md "Scheduling"), so the previous tick's count (iter_key, written by the kernel)
// predicts the next one. k_team_order sorts the robots by that key (stable counting sort, hardest first)
// and lays the sorted list out over the team slots:
//   sorted      slot s <- rank s: waves hold robots of like difficulty, the hard half of the blocks is
//               dispatched first;
//   interleaved even blocks take ranks from the hard end, odd blocks from the easy end, so neighbouring
//               blocks (which share CUs) pair a hard block with an easy one;
//   spread      the first wave of every block (one block = one CU at one wave per SIMD) takes the 4 x blocks
//               hardest robots, the other three waves the rest in order: the kernel ends with the slowest
//               wave, and a hard wave whose CU-mates finish early runs its last iterations alone on the CU
//               (memory pipeline and L1 no longer shared).
// Every robot keeps its own arithmetic whatever slot it lands in, so the order changes no result.
#include "nmpc_kernels.hpp"

namespace nmpc {

namespace {

constexpr int kOrderThreads = 1024;
constexpr int kOrderBins = 32;  // keys clamp to [0, 31] (IPM iterations; iter_max reaches 50 only on failures)

__global__ __launch_bounds__(kOrderThreads) void k_team_order(const int* __restrict__ key, int B, int layout,
                                                               int* __restrict__ sorted, int* __restrict__ order)
{
    // cnt[bin][thread]: private column per thread, then one exclusive scan in (bin descending, thread) order
    __shared__ unsigned cnt[kOrderBins][kOrderThreads];
    __shared__ unsigned part[kOrderThreads];
    const int t = threadIdx.x;
    const int E = (B + kOrderThreads - 1) / kOrderThreads;
    const int i0 = min(B, t * E), i1 = min(B, i0 + E);
    for (int b = 0; b < kOrderBins; b++) cnt[b][t] = 0;
    for (int i = i0; i < i1; i++) {
        const int k = min(max(key[i], 0), kOrderBins - 1);
        cnt[kOrderBins - 1 - k][t]++;
    }
    __syncthreads();
    // flattened index f = bin * T + thread; thread t scans f in [32 t, 32 t + 32)
    unsigned loc[kOrderBins];
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < kOrderBins; j++) {
        const int f = t * kOrderBins + j;
        loc[j] = s;
        s += cnt[f / kOrderThreads][f % kOrderThreads];
    }
    part[t] = s;
    __syncthreads();
    // Hillis-Steele inclusive scan of the partial sums
    for (int d = 1; d < kOrderThreads; d <<= 1) {
        const unsigned v = (t >= d) ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const unsigned base = part[t] - s;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kOrderBins; j++) {
        const int f = t * kOrderBins + j;
        cnt[f / kOrderThreads][f % kOrderThreads] = base + loc[j];
    }
    __syncthreads();
    int* dst = (layout == NMPC_SCHED_SORTED) ? order : sorted;
    for (int i = i0; i < i1; i++) {
        const int k = min(max(key[i], 0), kOrderBins - 1);
        dst[cnt[kOrderBins - 1 - k][t]++] = i;
    }
    if (layout == NMPC_SCHED_SORTED) return;
    __threadfence_block();
    __syncthreads();
    if (layout == NMPC_SCHED_SPREAD) {
        // wave-0 slots (s % 16 < 4) of block j take ranks 4 j .. 4 j + 3; every other slot follows in slot
        // order after the n0 wave-0 slots (only the last block can be partial)
        const int nb = (B + 15) >> 4;
        const int n0 = 4 * (nb - 1) + min(4, B - 16 * (nb - 1));
        for (int sl = t; sl < B; sl += kOrderThreads) {
            const int j = sl >> 4, w = sl & 15;
            order[sl] = sorted[(w < 4) ? 4 * j + w : n0 + sl - 4 * (j + 1)];
        }
        return;
    }
    // interleaved: slot s in block j = s / 16 (16 teams per block); even blocks count up from the hardest
    // rank, odd blocks down from the easiest (only the last block can be partial, so both runs are dense)
    for (int sl = t; sl < B; sl += kOrderThreads) {
        const int j = sl >> 4, w = sl & 15;
        const int q = (j >> 1) * 16 + w;
        order[sl] = sorted[(j & 1) ? B - 1 - q : q];
    }
}

// Node ticks (nmpc_batch_node_tick): the same stable counting sort with one more bin below every active one. The
// robots with active[i] != 0 come first -- hardest first by key when `sorted`, in index order otherwise (one bin) --
// and the others follow in index order; n_active[0] receives the count of the active ones, which is where the
// inactive bin starts.
constexpr int kNodeBins = kOrderBins + 1;

__global__ __launch_bounds__(kOrderThreads) void k_node_order(const int* __restrict__ key,
                                                               const unsigned char* __restrict__ active, int B,
                                                               int sorted, int* __restrict__ order,
                                                               int* __restrict__ n_active)
{
    __shared__ unsigned cnt[kNodeBins][kOrderThreads];
    __shared__ unsigned part[kOrderThreads];
    const int t = threadIdx.x;
    const int E = (B + kOrderThreads - 1) / kOrderThreads;
    const int i0 = min(B, t * E), i1 = min(B, i0 + E);
    auto bin_of = [&](int i) -> int {
        if (!active[i]) return kNodeBins - 1;
        return sorted ? kOrderBins - 1 - min(max(key[i], 0), kOrderBins - 1) : 0;
    };
    for (int b = 0; b < kNodeBins; b++) cnt[b][t] = 0;
    for (int i = i0; i < i1; i++) cnt[bin_of(i)][t]++;
    __syncthreads();
    // flattened index f = bin * T + thread; thread t scans f in [33 t, 33 t + 33)
    unsigned loc[kNodeBins];
    unsigned s = 0;
#pragma unroll
    for (int j = 0; j < kNodeBins; j++) {
        const int f = t * kNodeBins + j;
        loc[j] = s;
        s += cnt[f / kOrderThreads][f % kOrderThreads];
    }
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < kOrderThreads; d <<= 1) {
        const unsigned v = (t >= d) ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    const unsigned base = part[t] - s;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kNodeBins; j++) {
        const int f = t * kNodeBins + j;
        cnt[f / kOrderThreads][f % kOrderThreads] = base + loc[j];
    }
    __syncthreads();
    if (t == 0) n_active[0] = (int)cnt[kNodeBins - 1][0];  // (before thread 0's own scatter advances it)
    for (int i = i0; i < i1; i++) order[cnt[bin_of(i)][t]++] = i;
}

// the resident state's elementwise kernels (nmpc_batch_init_iterate, nmpc_batch_forget_warm)
__global__ void k_init_iterate(float* xbar, float* ubar, float* carried, unsigned char* warm, int B, int stride, int N,
                               int nx, int nu, int nbx, int mode)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    warm[i] = 0;  // the next solve starts its IPM cold
    for (int k = 0; k <= N; k++)
        for (int j = 0; j < nx; j++)
            xbar[((size_t)k * nx + j) * stride + i] = (mode == 0 && j == 2) ? 3.14159265358979323846f : 0.0f;
    for (int k = 0; k < N; k++)
        for (int j = 0; j < nu; j++) ubar[((size_t)k * nu + j) * stride + i] = 0.0f;
    // create semantics start the wrapper's x0 vel-refs at zero (the member struct is value-initialised); a reset
    // (reset_mpc -> {name}_acados_reset) leaves them, as the reference does and as the solve's reset mask does
    if (mode == 0)
        for (int j = 0; j < nbx; j++) carried[(size_t)j * stride + i] = 0.0f;
}

__global__ void k_forget_warm(unsigned char* warm, const unsigned char* mask, int B)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B && (!mask || mask[i])) warm[i] = 0;
}

}  // namespace

hipError_t launch_init_iterate(float* xbar, float* ubar, float* carried, unsigned char* warm, int B, int stride, int N,
                               int nx, int nu, int nbx, int mode, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_iterate, dim3((B + 255) / 256), dim3(256), 0, stream, xbar, ubar, carried, warm, B,
                       stride, N, nx, nu, nbx, mode);
    return hipGetLastError();
}

hipError_t launch_forget_warm(unsigned char* warm, const unsigned char* mask, int B, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_forget_warm, dim3((B + 255) / 256), dim3(256), 0, stream, warm, mask, B);
    return hipGetLastError();
}

hipError_t launch_node_order(const int* key, const unsigned char* active, int B, int sorted, int* order, int* n_active,
                             hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_node_order, dim3(1), dim3(kOrderThreads), 0, stream, key, active, B, sorted, order, n_active);
    return hipGetLastError();
}

hipError_t launch_team_order(const int* key, int B, int layout, int* sorted, int* order, hipStream_t stream)
{
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_team_order, dim3(1), dim3(kOrderThreads), 0, stream, key, B, layout, sorted, order);
    return hipGetLastError();
}

}  // namespace nmpc
