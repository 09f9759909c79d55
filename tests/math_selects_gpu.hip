// tests/math_selects_gpu.hip — the device half of the check of fg_phi_med / fg_softplus_max (feedback_gnn_amd/csrc/fgnn_math_ranged.h).
//
// tests/math_select_check.c proves on the CPU that the median / maximum forms return the bits of fg_phi / fg_softplus.  On the device
// the forms are other instructions (v_med3_f32, v_max_f32 where the CPU composes min and max), so this program evaluates both forms
// and the fgnn_math.h routines ON THE DEVICE, on the inputs where the selects switch, and counts differing bit patterns:
//   phi      every float of xc in [13.9, 14.8] (all of the band where the computed log1p exceeds xc and a plain max would fail) and a
//            stride-257 walk of the whole clip range [8.5e-8, 16.635532];
//   softplus every float of |t| in [13.9, 16.3] (the threshold and the band where exp(t) != log1p(exp(t))) and of |t| in [86.9, 87.1]
//            (the flush of the exponential), both signs, and a stride-4099 walk of every finite float of both signs.
// It also forms the CRC-32 of the device's outputs and of the host build's fg_phi / fg_softplus on the same inputs (this file's host
// pass compiles the same header): the two must be equal.  Prints one line per routine; exits 1 on any difference.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-slp-vectorize tests/math_selects_gpu.hip
// (the flags of feedback_gnn_amd/csrc/Makefile).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../feedback_gnn_amd/csrc/fgnn_math_ranged.h"

template <int FN>
__global__ void __launch_bounds__(256) eval(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, unsigned n, unsigned* __restrict__ ndiff)
{
    FG_LOG_TAB_SETUP();
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float x = fg_u2f(in[i]);
    const uint32_t got = fg_f2u(FN == 0 ? fg_phi_med(x) : fg_softplus_max(x));
    const uint32_t want = fg_f2u(FN == 0 ? fg_phi(x) : fg_softplus(x));
    out[i] = got;
    if (got != want) atomicAdd(ndiff, 1u);
}

static uint32_t bits(float x) { return fg_f2u(x); }

static void walk(std::vector<uint32_t>& v, uint32_t lo, uint32_t hi, uint32_t stride)
{
    for (uint64_t u = lo; u <= hi; u += stride) v.push_back((uint32_t)u);
}

static uint32_t crc32(const std::vector<uint32_t>& words)
{
    static uint32_t tab[256];
    if (!tab[1])
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
            tab[i] = c;
        }
    uint32_t c = 0xffffffffu;
    for (uint32_t w : words)
        for (int b = 0; b < 4; ++b) c = tab[(c ^ (w >> (8 * b))) & 0xffu] ^ (c >> 8);
    return ~c;
}

template <int FN>
static int run(const char* name, const std::vector<uint32_t>& in, unsigned long in_band)
{
    const unsigned n = (unsigned)in.size();
    uint32_t *d_in, *d_out;
    unsigned* d_diff;
    if (hipMalloc(&d_in, n * 4ul) != hipSuccess || hipMalloc(&d_out, n * 4ul) != hipSuccess || hipMalloc(&d_diff, 4) != hipSuccess) return 3;
    if (hipMemcpy(d_in, in.data(), n * 4ul, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_diff, 0, 4) != hipSuccess) return 3;
    hipLaunchKernelGGL(eval<FN>, dim3((n + 255u) / 256u), dim3(256), 0, 0, d_in, d_out, n, d_diff);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 3;
    std::vector<uint32_t> out(n), host(n);
    unsigned ndiff = 0;
    if (hipMemcpy(out.data(), d_out, n * 4ul, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&ndiff, d_diff, 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_diff);
    for (unsigned i = 0; i < n; ++i) host[i] = fg_f2u(FN == 0 ? fg_phi(fg_u2f(in[i])) : fg_softplus(fg_u2f(in[i])));
    const uint32_t cd = crc32(out), ch = crc32(host);
    std::printf("%s: %u inputs (%lu in the select bands), %u differences on the device, crc device %08x host %08x\n", name, n, in_band, ndiff, cd, ch);
    return (ndiff != 0 || cd != ch) ? 1 : 0;
}

int main()
{
    std::vector<uint32_t> phi_in, sp_in;
    walk(phi_in, bits(13.9f), bits(14.8f), 1);
    const unsigned long phi_band = phi_in.size();
    walk(phi_in, bits(FG_PHI_MIN), bits(FG_PHI_MAX), 257);
    phi_in.push_back(bits(FG_PHI_MAX));
    for (uint32_t sign : {0x00000000u, 0x80000000u}) {
        walk(sp_in, sign | bits(13.9f), sign | bits(16.3f), 1);
        walk(sp_in, sign | bits(86.9f), sign | bits(87.1f), 1);
    }
    const unsigned long sp_band = sp_in.size();
    walk(sp_in, 0x00000000u, 0x7f7fffffu, 4099);
    walk(sp_in, 0x80000000u, 0xff7fffffu, 4099);
    sp_in.push_back(0x7f7fffffu);
    sp_in.push_back(0xff7fffffu);
    const int r0 = run<0>("phi", phi_in, phi_band);
    if (r0 == 3) return 3;
    const int r1 = run<1>("softplus", sp_in, sp_band);
    return r0 | r1;
}
