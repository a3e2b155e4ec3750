// what a vector compare (VOPC, and VOP3 with a scalar destination) and the carry-out of v_sub_co write for INACTIVE lanes on
// gfx950: zero, or what the register held?  k_lz_parse's chain step relies on zero (kernels_parse.h, PZ_RSTEP): vcc after a compare
// is a subset of exec, also when exec is empty.  Every destination is preset to all ones, exec is cut down to `mask`, the three
// instructions are true (borrow) in every lane that runs them.  Expected: all three equal `mask`.
//   hipcc --offload-arch=gfx950 -O2 -o tools/ubench/vopc_inactive.bin tools/ubench/vopc_inactive.hip && tools/ubench/vopc_inactive.bin
#include <hip/hip_runtime.h>
#include <cstdio>
__global__ void k(unsigned long long mask, unsigned long long* out) {
    unsigned long long r_vcc, r_sdst, r_co, save;
    unsigned v = threadIdx.x, d;
    asm volatile(
        "s_mov_b64 %[save], exec\n\t"
        "s_mov_b64 vcc, -1\n\t"
        "s_mov_b64 %[rs], -1\n\t"
        "s_mov_b64 %[rc], -1\n\t"
        "s_mov_b64 exec, %[m]\n\t"
        "v_cmp_eq_u32 vcc, %[v], %[v]\n\t"
        "v_cmp_eq_u32_e64 %[rs], %[v], %[v]\n\t"
        "v_sub_co_u32_e64 %[d], %[rc], 0, 1\n\t"
        "s_nop 4\n\t"
        "s_mov_b64 %[rv], vcc\n\t"
        "s_mov_b64 exec, %[save]\n\t"
        : [rv] "=&s"(r_vcc), [rs] "=&s"(r_sdst), [rc] "=&s"(r_co), [save] "=&s"(save), [d] "=&v"(d)
        : [m] "s"(mask), [v] "v"(v)
        : "vcc");
    if (threadIdx.x == 0) {
        out[0] = r_vcc;
        out[1] = r_sdst;
        out[2] = r_co;
    }
}
int main() {
    const unsigned long long masks[4] = {0x0f0f0f0f00ff00ffull, 0ull, ~0ull, 0x8000000000000001ull};
    unsigned long long* d;
    if (hipMalloc(&d, 24) != hipSuccess) return 2;
    int bad = 0;
    for (int i = 0; i < 4; i++) {
        unsigned long long h[3] = {1, 2, 3};
        k<<<1, 64>>>(masks[i], d);
        if (hipMemcpy(h, d, 24, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        const bool ok = h[0] == masks[i] && h[1] == masks[i] && h[2] == masks[i];
        bad += !ok;
        printf("exec %016llx: v_cmp vcc %016llx  v_cmp_e64 sdst %016llx  v_sub_co carry %016llx  %s\n", masks[i], h[0], h[1], h[2],
               ok ? "inactive lanes ZERO" : "inactive lanes KEPT");
    }
    return bad ? 1 : 0;
}
