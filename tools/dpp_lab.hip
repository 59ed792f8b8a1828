// tools/dpp_lab.hip -- developer probe (NOT product): what DPP wave shifts do as VOP2 source operands on gfx950, and how many
// wait states a DPP read needs after a VALU write of its source.  One wavefront; prints what each lane got.
//     hipcc --offload-arch=gfx950 -O2 -o dpp_lab tools/dpp_lab.hip && ./dpp_lab
// What it said (profiles/tile_settle_rounds.txt, section 3): v_subrev_co_u32_dpp D, vcc, A, B gives A[shifted] - B, like
// v_sub_co_u32_dpp; wave_shl:1 / wave_shr:1 cross the 16-lane rows, bound_ctrl:0 makes the lane without a source read 0; with ONE
// wait state after the write wave_shl:1 reads the old value in lanes 15, 31 and 47, with two every lane reads the new one.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>

// ---- 1. operands: x = 1000 - 10 * lane (descending) ---------------------------------------------------------------------
#define TAIL_A " row_mask:0xf bank_mask:0xf"
__global__ void operands(uint32_t* out, unsigned long long* masks) {
    const uint32_t lane = threadIdx.x;
    uint32_t x = 1000 - 10 * lane, zero = 0;
    uint32_t a = 0, b, c, d, e, f;
    unsigned long long m1, m2, m3;
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 wave_shr:1" TAIL_A : "+v"(a) : "v"(x));
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 wave_shr:1" TAIL_A " bound_ctrl:0" : "=&v"(b) : "v"(x));
    asm volatile("s_nop 1\n\tv_subrev_co_u32_dpp %0, vcc, %2, %2 wave_shr:1" TAIL_A " bound_ctrl:0\n\ts_mov_b64 %1, vcc" : "=&v"(c), "=&s"(m1) : "v"(x) : "vcc");
    asm volatile("s_nop 1\n\tv_sub_co_u32_dpp %0, vcc, %2, %2 wave_shl:1" TAIL_A " bound_ctrl:0\n\ts_mov_b64 %1, vcc" : "=&v"(d), "=&s"(m2) : "v"(x) : "vcc");
    asm volatile("s_nop 1\n\tv_subrev_co_u32_dpp %0, vcc, %2, %2 wave_shr:1" TAIL_A " bound_ctrl:0\n\t"
                 "v_subbrev_co_u32_dpp %0, vcc, %3, %3, vcc wave_shr:1" TAIL_A " bound_ctrl:0\n\ts_mov_b64 %1, vcc" : "=&v"(e), "=&s"(m3) : "v"(x), "v"(zero) : "vcc");
    asm volatile("s_nop 1\n\ts_mov_b64 vcc, 0\n\tv_cndmask_b32_dpp %0, %1, %1, vcc wave_shl:1" TAIL_A " bound_ctrl:0" : "=&v"(f) : "v"(x) : "vcc");
    out[lane] = a; out[64 + lane] = b; out[128 + lane] = c; out[192 + lane] = d; out[256 + lane] = e; out[320 + lane] = f;
    if (lane == 0) { masks[0] = m1; masks[1] = m2; masks[2] = m3; }
}
static int run_operands() {
    uint32_t* o; unsigned long long* m;
    if (hipMalloc(&o, 384 * 4) != hipSuccess || hipMalloc(&m, 24) != hipSuccess) return 1;
    operands<<<1, 64>>>(o, m);
    uint32_t h[384]; unsigned long long hm[3];
    if (hipMemcpy(h, o, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
    if (hipMemcpy(hm, m, sizeof hm, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    const char* names[6] = {"mov shr (old 0)", "mov shr bound_ctrl", "subrev shr = x - x[l-1]", "sub shl = x[l+1] - x", "subrev+subbrev shr", "cndmask shl (vcc 0)"};
    for (int k = 0; k < 6; ++k) { printf("%-26s", names[k]); for (int l = 0; l < 64; ++l) if (l < 3 || (l >= 14 && l <= 18) || (l >= 30 && l <= 33) || l >= 62) printf(" %d:%d", l, (int)h[k * 64 + l]); printf("\n"); }
    printf("vcc subrev shr %016llx | sub shl %016llx | 64-bit subrev shr %016llx\n", hm[0], hm[1], hm[2]);
    return 0;
}

// ---- 2. wait states between v_add_u32 x, 5000, x and a DPP read of x --------------------------------------------------------

#define TAIL " row_mask:0xf bank_mask:0xf bound_ctrl:0"
#define ONE(K, NOPS, CTRL, SLOT)                                                                          \
    { uint32_t y = x, r;                                                                                  \
      asm volatile("s_nop 7\n\tv_add_u32 %1, 5000, %1\n\t" NOPS "v_mov_b32_dpp %0, %1 " CTRL TAIL          \
                   : "=&v"(r), "+v"(y));                                                                  \
      out[((SLOT) * 8 + (K)) * 64 + lane] = r; }
#define ALL(CTRL, SLOT)                                                                                   \
    ONE(0, "", CTRL, SLOT) ONE(1, "s_nop 0\n\t", CTRL, SLOT) ONE(2, "s_nop 1\n\t", CTRL, SLOT) ONE(3, "s_nop 2\n\t", CTRL, SLOT) \
    ONE(4, "s_nop 3\n\t", CTRL, SLOT) ONE(5, "s_nop 4\n\t", CTRL, SLOT) ONE(6, "s_nop 5\n\t", CTRL, SLOT) ONE(7, "s_nop 6\n\t", CTRL, SLOT)
__global__ void wait_states(uint32_t* out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t x = 1000 - 10 * lane;
    ALL("quad_perm:[1,0,3,2]", 0)
    ALL("wave_shl:1", 1)
    ALL("wave_shr:1", 2)
}
static int run_wait_states() {
    uint32_t* o;
    if (hipMalloc(&o, 3 * 8 * 64 * 4) != hipSuccess) return 1;
    static uint32_t h[3 * 8 * 64];
    for (int rep = 0; rep < 3; ++rep) {
        wait_states<<<1, 64>>>(o);
        if (hipMemcpy(h, o, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
        const char* names[3] = {"quad_perm", "wave_shl:1", "wave_shr:1"};
        for (int s = 0; s < 3; ++s)
            for (int k = 0; k < 8; ++k) {
                int bad = 0, first = -1;
                for (int l = 0; l < 64; ++l) {
                    const int src = s == 0 ? (l ^ 1) : s == 1 ? l + 1 : l - 1;
                    const uint32_t want = (src < 0 || src > 63) ? 0u : 6000u - 10u * (uint32_t)src;
                    if (h[(s * 8 + k) * 64 + l] != want) { if (first < 0) first = l; ++bad; }
                }
                printf("rep %d %-10s wait states %d: %2d lanes stale (first %d)\n", rep, names[s], k, bad, first);
            }
    }
    return 0;
}

int main() { return run_operands() || run_wait_states(); }
