// Weight-pack plumbing shared by winograd24.hip and winograd44f.hip: the two small pack kernels and their host side,
// templated on the kernel's traits K (wino_plan.h) and its transform GROUP (wino_pack_group / f44_pack_group: one
// 512-thread workgroup writes one (tile, chunk) group = K::SLICES x 64 x 8 outputs of the forward or the backward pack).
#pragma once
#include "common.h"
#include "wino_plan.h"

namespace {

using WinoPackGroup = void (*)(const float* w, float* uf, float* ub, int Cout, int Cin, size_t nf, size_t nb, size_t group);

template <class K>
constexpr int WINO_PACK_BLOCKS = K::SLICES * K::CO * K::CK / 256;      // 256-output units per pack group (48 / 72)

template <class K>
inline int wino_pack_sizes(int Cout, int Cin, long* fwd_floats, long* bwd_floats) {
    *fwd_floats = (long)K::SLICES * rup(Cin, K::CK) * rup(Cout, K::CO);
    *bwd_floats = (long)K::SLICES * rup(Cout, K::CK) * rup(Cin, K::CO);
    return 0;
}

template <class K, WinoPackGroup GROUP>
__global__ __launch_bounds__(512) void wino_pack_kernel(const float* __restrict__ w, float* __restrict__ uf,
                                                        float* __restrict__ ub, int Cout, int Cin, size_t nf,
                                                        size_t nb) {
    GROUP(w, uf, ub, Cout, Cin, nf, nb, blockIdx.x);
}

// many layers in one launch; desc: device int64 [nlayers][8] rows
struct WinoPackDesc {
    const float* w;
    float* uf;
    float* ub;
    long long Cout, Cin, nf, nb, first_block;         // first_block in units of 256 outputs (WINO_PACK_BLOCKS per group)
};
template <class K, WinoPackGroup GROUP>
__global__ __launch_bounds__(512) void wino_pack_multi_kernel(const WinoPackDesc* __restrict__ desc, int nlayers) {
    const long long vb = (long long)blockIdx.x * WINO_PACK_BLOCKS<K>;
    int lo = 0, hi = nlayers;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (desc[mid].first_block <= vb) lo = mid; else hi = mid;
    }
    const WinoPackDesc d = desc[lo];
    GROUP(d.w, d.uf, d.ub, (int)d.Cout, (int)d.Cin, (size_t)d.nf, (size_t)d.nb,
          (size_t)((vb - d.first_block) / WINO_PACK_BLOCKS<K>));
}

template <class K, WinoPackGroup GROUP>
int wino_pack_weights(const float* w_oihw, float* u_fwd, float* u_bwd, int Cout, int Cin, void* stream) {
    long nf, nb;
    wino_pack_sizes<K>(Cout, Cin, &nf, &nb);
    if (!u_bwd) nb = 0;
    hipLaunchKernelGGL((wino_pack_kernel<K, GROUP>), dim3((unsigned)((nf + nb) / (K::SLICES * K::CO * K::CK))), dim3(512), 0,
                       (hipStream_t)stream, w_oihw, u_fwd, u_bwd, Cout, Cin, (size_t)nf, (size_t)nb);
    VF_RETURN_LAST_ERROR();
}

template <class K, WinoPackGroup GROUP>
int wino_pack_weights_multi(const void* desc, int nlayers, long total_blocks, void* stream) {
    if (nlayers <= 0 || total_blocks <= 0) return 0;
    hipLaunchKernelGGL((wino_pack_multi_kernel<K, GROUP>), dim3((unsigned)(total_blocks / WINO_PACK_BLOCKS<K>)), dim3(512), 0,
                       (hipStream_t)stream, (const WinoPackDesc*)desc, nlayers);
    VF_RETURN_LAST_ERROR();
}

}  // namespace
