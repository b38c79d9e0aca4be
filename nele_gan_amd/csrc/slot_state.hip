// The one reset kernel of the per-stream slot states (slot_state.h).
#include "slot_state.h"

namespace {

struct SlotHdr {
    int v[8];
};

// grid (S), block 256.  hdr.v: the geometry header's values, nhdr of them written (0: no header write); first: a reset record's first int
__global__ void slot_reset_kernel(unsigned char* __restrict__ state, long long hdr_bytes, long long rec_bytes, int S,
                                  const unsigned char* __restrict__ slots, int nhdr, SlotHdr hdr, int first) {
    const int b = blockIdx.x, t = threadIdx.x;
    if (nhdr && b == 0 && t < SLOT_GEOM_HDR_BYTES / 4) {
        int v = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) v = (t == i && i < nhdr) ? hdr.v[i] : v;
        reinterpret_cast<int*>(state)[t] = v;
    }
    if (b >= S || (slots && !slots[b])) return;
    uint4* r = reinterpret_cast<uint4*>(state + hdr_bytes + (size_t)b * rec_bytes);
    for (long long i = t; i < rec_bytes / 16; i += blockDim.x) r[i] = make_uint4(i == 0 ? (unsigned)first : 0u, 0u, 0u, 0u);
}

}  // namespace

int slot_state_reset(const char* name, void* state, long long hdr_bytes, long long rec_bytes, int S, const unsigned char* slots, int nhdr,
                     const int* hdr, void* stream, int first) {
    nhdr = nhdr < 8 ? nhdr : 8;
    SlotHdr h{};
    for (int i = 0; i < nhdr; ++i) h.v[i] = hdr[i];
    hipLaunchKernelGGL(slot_reset_kernel, dim3(S), dim3(256), 0, as_stream(stream), (unsigned char*)state, hdr_bytes, rec_bytes, S, slots, nhdr, h,
                       first);
    NELE_CHECK_LAUNCH(name);
    return NELE_OK;
}
