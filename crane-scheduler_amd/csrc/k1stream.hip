// k1stream.hip — the node pass fused with the step tables, streamed (K1 for large N): the kernel
// of its own launch.  The body is k1stream_body.hpp's.
#include <hip/hip_runtime.h>

#include "k1stream_body.hpp"

namespace crane {

template <int PD, int PR, bool FULL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PD * PR <= 24 ? K1S_WAVES : 1)))
void k1_stream_steps(K1Args a, K1Step step) {
    __shared__ K1Lds<PD, PR> lds;
    k1_stream_body<PD, PR, FULL, (int)sizeof(K1Args) + (int)sizeof(K1Step)>(a, step, blockIdx.x, gridDim.x, lds);
}

template <int PD, int PR, bool FULL = false>
static hipError_t launch_t(const K1Args& a, const K1Step& sa, hipStream_t st) {
    const unsigned grid = (unsigned)((a.N + 255) / 256);
    return klaunch("k1_stream_steps", k1_stream_steps<PD, PR, FULL>, dim3(grid), dim3(256), 0, st, a, sa);
}

hipError_t launch_stream_steps(int pd, int pr, const K1Args& a, const K1Step& sa, hipStream_t st) {
    if (a.N <= 0) return hipSuccess;
    if (K1S_FULL && a.pol.npd == 4 && a.pol.npr == 6 && a.pol.n_win == kFullWin) return launch_t<4, 6, true>(a, sa, st);
    if (pd <= 4 && pr <= 6) return launch_t<4, 6>(a, sa, st);
    if (pd <= 8 && pr <= 8) return launch_t<8, 8>(a, sa, st);
    return launch_t<16, 16>(a, sa, st);
}

}  // namespace crane
