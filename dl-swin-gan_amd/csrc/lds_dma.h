// 16-B vector types, global -> LDS DMA and transposed LDS reads of the conv and f16x3 units.
#pragma once
#include "dlcs_common.h"

namespace {
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s_t;

// global -> LDS DMA of 16 B per lane to (wave-uniform lds_addr) + 16 * lane.
// Issued from inline asm on purpose: hipcc cannot tell which LDS buffer a
// builtin DMA writes and waits vmcnt(0) before every later ds_read, which would
// serialise the prefetch of patch p+1 with the MFMAs of patch p.  The caller
// waits (s_waitcnt vmcnt(0)) before the barrier that publishes the buffer.
DLCS_DEV void glds16(const void* gptr, unsigned lds_addr) {
    // m0 is saved and restored around the DMA (the compiler may keep a value in it)
    unsigned saved;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(saved) : "v"(gptr), "s"(__builtin_amdgcn_readfirstlane(lds_addr)) : "memory");
}

// the same DMA with a wave-uniform 64-bit base in SGPRs and a per-lane 32-bit
// byte offset (the saddr form: no per-lane 64-bit address arithmetic)
DLCS_DEV void glds16_s(const void* sbase, unsigned voff, unsigned lds_addr) {
    unsigned saved;
    const unsigned long long sb = (unsigned long long)(uintptr_t)sbase;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)sb);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(sb >> 32));
    const unsigned long long sbu = ((unsigned long long)hi << 32) | lo;
    // s_nop 4: the saddr pair may come straight from v_readfirstlane
    // (cdna_hip_programming.md 5.7 item 2)
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 4\n\tglobal_load_lds_dwordx4 %1, %2\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(saved) : "v"(voff), "s"(sbu), "s"(__builtin_amdgcn_readfirstlane(lds_addr)) : "memory");
}

DLCS_DEV unsigned lds_offset(const void* p) {
    return (unsigned)(uintptr_t)((const __attribute__((address_space(3))) char*)(p));
}

DLCS_DEV bf16x8_t tr_read16(const bf16* p0, const bf16* p1) {
    const v4s r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(const_cast<bf16*>(p0)));
    const v4s r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_t*)(const_cast<bf16*>(p1)));
    typedef short v8s __attribute__((ext_vector_type(8)));
    const v8s both = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
    return __builtin_bit_cast(bf16x8_t, both);
}

}  // namespace
