// Batch assembly from a device-resident view store (view_fusion_amd/data.py: ViewStore): the reference loader's
// process_sample + collate + .to(device) (data/nmr_dataset.py:10-52, experiment.py:271-284) as ONE launch.
//
// The store is a dataset split as planar uint8 [N][24][3][H][W].  A sample's target, conditioning views and angle are a
// function of (seed, sample id) alone -- the data draws of rng.h (kind 4) turned into view indices by batch_plan.h -- so
// building a batch is a permuted gather with a uint8 -> float conversion.
//
// Grid (24, B): workgroup (slot, b) writes one output image of sample b -- slot 0 the target y_0[b], slot k >= 1 the
// conditioning view y_cond[b][k - 1] (with `relative`: 6 channels, the reference view src[1] in front); with `all` the
// plan is the identity and slot v writes view v of objects[b] (store.all_views).  Every workgroup derives its sample's
// plan itself: 13 lanes make the 13 Philox calls, one lane shuffles, all read the result from LDS.
// A pixel is table[byte], table[i] = i / 255 correctly rounded (__fdiv_rn) = np.float32(i) / np.float32(255).
// uchar4 loads, float4 stores (H * W % 4 == 0); every store offset is 64-bit; no atomics; an object index outside
// [0, N) reads nothing and fills its outputs with NaN.
#include "common.h"
#include "batch_plan.h"
#include "vf_hip.h"

namespace {

__device__ __forceinline__ void convert_plane(const uchar4* __restrict__ in, float4* __restrict__ out, int n4,
                                              const float* tab) {
    for (int i = threadIdx.x; i < n4; i += 256) {
        const uchar4 u = in[i];
        out[i] = make_float4(tab[u.x], tab[u.y], tab[u.z], tab[u.w]);
    }
}

__global__ __launch_bounds__(256) void batch_assemble_kernel(
    const uchar4* __restrict__ store, long long N, int n4 /* 3 H W / 4: float4s of one view */, unsigned long long seed,
    const long long* __restrict__ ids, const long long* __restrict__ objects, int train, int relative, int all,
    float4* __restrict__ y_0, float4* __restrict__ y_cond, float* __restrict__ angle,
    long long* __restrict__ objects_out) {
    __shared__ float tab[256];
    __shared__ uint32_t words[VF_DATA_WORDS];
    __shared__ VfViewPlan plan;
    __shared__ long long object;
    const int slot = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;

    tab[tid] = __fdiv_rn((float)tid, 255.0f);
    if (!all && tid < VF_DATA_BLOCKS)
        vf_rng_words(seed, (unsigned long long)ids[b], VF_RNG_DATA, 0, (uint32_t)tid, words + 4 * tid);
    __syncthreads();
    if (tid == 0) {
        if (all) vf_batch_identity_plan(&plan);
        else vf_batch_view_plan(words, train, &plan);
        object = objects ? objects[b] : vf_batch_object(words, (uint32_t)N);
    }
    __syncthreads();

    const long long obj = object;
    const bool ok = obj >= 0 && obj < N;
    if (slot == 0 && tid == 0 && !all) {
        if (angle)
            angle[b] = !ok ? __int_as_float(0x7fc00000)
                           : vf_batch_angle(relative ? (int)plan.q1 - (int)plan.q0 : (int)plan.target);
        if (objects_out) objects_out[b] = obj;
    }

    const int C4 = relative && slot > 0 ? 2 * n4 : n4;           // float4s of this workgroup's output image
    float4* out;
    if (all) out = y_cond + ((long long)b * VF_VIEWS + slot) * n4;
    else if (slot == 0) out = y_0 + (long long)b * n4;
    else out = y_cond + ((long long)b * (VF_VIEWS - 1) + (slot - 1)) * C4;
    if (!ok) {
        const float nan = __int_as_float(0x7fc00000);
        for (int i = tid; i < C4; i += 256) out[i] = make_float4(nan, nan, nan, nan);
        return;
    }
    const uchar4* views = store + obj * VF_VIEWS * (long long)n4;
    const int v = slot == 0 ? plan.target : plan.src[slot];      // (identity plan: target = 0 = src[0])
    if (relative && slot > 0) {
        convert_plane(views + (long long)plan.src[1] * n4, out, n4, tab);
        out += n4;
    }
    convert_plane(views + (long long)v * n4, out, n4, tab);
}

}  // namespace

extern "C" {

int vf_batch_assemble(const unsigned char* store, long N, int H, int W, unsigned long long seed, const long long* ids,
                      const long long* objects, int B, int train, int relative, int all, float* y_0, float* y_cond,
                      float* angle, long long* objects_out, void* stream) {
    if (B <= 0) return 0;
    const long long HW = (long long)H * W;
    if (!store || N < 1 || N > 0xffffffffL || H < 1 || W < 1 || (HW & 3) || 3 * HW / 4 > 0x7fffffffLL || B > 65535 ||
        !y_cond)
        return (int)hipErrorInvalidValue;
    if (all ? !objects : (!ids || !y_0 || !angle)) return (int)hipErrorInvalidValue;
    if (all) relative = 0;                                       // 24 plain views per object
    hipLaunchKernelGGL(batch_assemble_kernel, dim3(VF_VIEWS, B), dim3(256), 0, (hipStream_t)stream,
                       (const uchar4*)store, (long long)N, (int)(3 * HW / 4), seed, ids, objects, train, relative, all,
                       (float4*)y_0, (float4*)y_cond, angle, objects_out);
    VF_RETURN_LAST_ERROR();
}

// Host mirror: HOST pointers, no stream.  The product needs it, not only the tests: view_count must be known on the host
// without a sync (the Trainer keys its captured graphs on it).
int vf_batch_host_plan(unsigned long long seed, const long long* ids, int B, int train, int lo, int hi, long N,
                       const long long* objects, int* src, int* target, int* q01, int* second, long long* view_count,
                       long long* object) {
    if (B < 0 || lo < 1 || hi < lo || hi > VF_VIEWS - 1 || N < 1 || N > 0xffffffffL) return (int)hipErrorInvalidValue;
    for (int b = 0; b < B; ++b) {
        uint32_t w[VF_DATA_WORDS];
        VfViewPlan plan;
        vf_batch_words(seed, (unsigned long long)ids[b], w);
        vf_batch_view_plan(w, train, &plan);
        const long long obj = objects ? objects[b] : vf_batch_object(w, (uint32_t)N);
        if (obj < 0 || obj >= N) return (int)hipErrorInvalidValue;
        for (int i = 0; i < VF_VIEWS; ++i) src[b * VF_VIEWS + i] = plan.src[i];
        target[b] = plan.target;
        q01[2 * b] = plan.q0;
        q01[2 * b + 1] = plan.q1;
        second[b] = plan.second;
        view_count[b] = vf_batch_view_count(w, lo, hi);
        object[b] = obj;
    }
    return 0;
}

}  // extern "C"
