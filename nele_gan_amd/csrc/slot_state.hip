// The one reset kernel of the per-stream slot states (slot_state.h).
#include "slot_state.h"

namespace {

// grid (S), block 256.  hdr.x .. hdr.w: the geometry header's values, nhdr of them written (0: no header write)
__global__ void slot_reset_kernel(unsigned char* __restrict__ state, long long hdr_bytes, long long rec_bytes, int S,
                                  const unsigned char* __restrict__ slots, int nhdr, int4 hdr) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (nhdr && b == 0 && t < SLOT_GEOM_HDR_BYTES / 4) {
        const int v = t == 0 ? hdr.x : (t == 1 ? hdr.y : (t == 2 ? hdr.z : hdr.w));
        reinterpret_cast<int*>(state)[t] = t < nhdr ? v : 0;
    }
    if (b >= S || (slots && !slots[b])) return;
    uint4* r = reinterpret_cast<uint4*>(state + hdr_bytes + (size_t)b * rec_bytes);
    for (long long i = t; i < rec_bytes / 16; i += blockDim.x) r[i] = make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace

int slot_state_reset(const char* name, void* state, long long hdr_bytes, long long rec_bytes, int S, const unsigned char* slots, int nhdr,
                     const int* hdr, void* stream) {
    nhdr = nhdr < 4 ? nhdr : 4;
    int v[4] = {0, 0, 0, 0};
    for (int i = 0; i < nhdr; ++i) v[i] = hdr[i];
    hipLaunchKernelGGL(slot_reset_kernel, dim3(S), dim3(256), 0, as_stream(stream), (unsigned char*)state, hdr_bytes, rec_bytes, S, slots, nhdr,
                       make_int4(v[0], v[1], v[2], v[3]));
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
