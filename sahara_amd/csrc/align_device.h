// align_device.h — the device-side accessors that the kernels running
// align_core.h's table share (align.hip kAlignHits, rescue.hip kRescueScan):
// 3-bit-plane blocks behind a buffer descriptor, and a lane's table in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "align_core.h"

namespace sahara {
namespace {

// One wave per workgroup in both kernels: the table of K = 8 is 19.1 KB of LDS per workgroup.
constexpr uint32_t kAlignLanes = 64;

// (as search_text.hip bufferOf: loads past the end return 0 without a memory request)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t alignBufferOf(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, (int)bytes, 0x00020000);
}

struct BufBlocks {  // block b of a 3-bit-plane array behind a buffer descriptor
    __amdgpu_buffer_rsrc_t buf;
    __device__ __forceinline__ Planes3 operator()(uint32_t b) const {
        const auto v = __builtin_amdgcn_raw_buffer_load_b128(buf, b * 16u, 0, 0);
        return {v[0], v[1], v[2]};
    }
};

// The table ((K + 1)(2K + 1) 16-bit entries per lane) lane-interleaved in LDS:
// entry k of this lane at lds[k * kAlignLanes + lane], two lanes per bank word.
struct LaneTable {
    int16_t* t;
    __device__ __forceinline__ int operator()(int k) const { return t[k * (int)kAlignLanes]; }
    __device__ __forceinline__ void set(int k, int v) { t[k * (int)kAlignLanes] = (int16_t)v; }
};
// its bytes for one workgroup
inline size_t alignTableBytes(uint32_t maxErr, bool edit) {
    const uint32_t band = edit ? 2 * maxErr + 1 : 1;
    return (size_t)(maxErr + 1) * band * kAlignLanes * sizeof(int16_t);
}

}  // namespace
}  // namespace sahara
