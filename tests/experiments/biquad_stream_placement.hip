// Where the four waves of a biquad_stream_kernel workgroup sit: the SIMD of hardware waves 0..3 of every workgroup of a CU,
// from the HW_ID each wave leaves at the end of the launch (MI_STREAM_PROBE_END, slot 9: wave 3:0, SIMD 5:4, CU 11:8,
// SH 12, SE 15:13; slot 10: the XCD).  The pipeline position of a wave decides when it starts and when it runs dry, so
// positions that share a SIMD across the workgroups of a CU leave SIMDs idle while the launch fills and drains.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -DMI_BIQUAD_PROBE -I include -I lsp-dsp-units_amd/csrc \
//        tests/experiments/biquad_stream_placement.hip lsp-dsp-units_amd/csrc/runtime.hip -o tests/experiments/biquad_stream_placement_probe
// Run:   biquad_stream_placement_probe [channels = 1024] [blocks = 20]
#include "../../lsp-dsp-units_amd/csrc/biquad.hip"
#include <algorithm>
#include <cstdio>
#include <map>
#include <string>

int main(int argc, char **argv)
{
    const uint32_t C = (argc > 1) ? atoi(argv[1]) : 1024, NS = 8;
    const int K = (argc > 2) ? atoi(argv[2]) : 20;
    const size_t n = 4096;
    const int NWV = 4;
    if (C > 1024 || K > 128) { printf("at most 1024 channels and 128 blocks\n"); return 1; }
    mi_biquad_bank_t *bank = nullptr;
    if (mi_biquad_bank_create(&bank, C, NS) != MI_OK) { printf("create: %s\n", mi_dspu_last_error()); return 1; }
    std::vector<mi_biquad_x1_t> ch(size_t(C) * NS);
    for (auto &q : ch) { q.b0 = 0.25f; q.b1 = 0.5f; q.b2 = 0.25f; q.a1 = 0.1f; q.a2 = -0.05f; q.p0 = q.p1 = q.p2 = 0.0f; }
    mi_biquad_bank_set_all_chains(bank, ch.data(), NS, 1);
    float *in, *out;
    const int ring = 4;
    if (hipMalloc(&in, ring * C * n * sizeof(float)) != hipSuccess || hipMalloc(&out, ring * C * n * sizeof(float)) != hipSuccess) return 1;
    (void)hipMemset(in, 0, ring * C * n * sizeof(float));
    std::vector<float *> po(K);
    std::vector<const float *> pi(K);
    for (int k = 0; k < K; ++k) { po[k] = out + size_t(k % ring) * C * n; pi[k] = in + size_t(k % ring) * C * n; }
    for (int rep = 0; rep < 3; ++rep)
        if (mi_biquad_bank_process_blocks(bank, po.data(), pi.data(), K, n, n, n, nullptr) != MI_OK) { printf("%s\n", mi_dspu_last_error()); return 1; }
    if (hipDeviceSynchronize() != hipSuccess) { printf("the launch failed\n"); return 1; }
    std::vector<unsigned long long> h(4096 * 16 * 2);
    (void)hipMemcpyFromSymbol(h.data(), HIP_SYMBOL(g_probe), h.size() * sizeof(h[0]));

    struct wg { unsigned long long entry; uint32_t b; int simd[4]; };
    std::map<unsigned, std::vector<wg>> cu;
    for (uint32_t b = 0; b < C; ++b)
    {
        const unsigned hw = unsigned(h[b * NWV * 32 + 9]), xcc = unsigned(h[b * NWV * 32 + 10]) & 0xf;
        const unsigned key = (xcc << 12) | (((hw >> 13) & 7) << 8) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15);
        wg g;
        g.entry = h[b * NWV * 32];
        g.b = b;
        for (int w = 0; w < NWV; ++w) g.simd[w] = int((h[(b * NWV + w) * 32 + 9] >> 4) & 3);
        cu[key].push_back(g);
    }
    // a CU's pattern: the SIMDs of waves 0..3, workgroup after workgroup in the order of entry
    std::map<std::string, int> patterns;
    int same = 0, per_simd_one_each = 0, cus = 0, wave0_shared = 0;
    for (auto &kv : cu)
    {
        auto &v = kv.second;
        std::sort(v.begin(), v.end(), [](const wg &a, const wg &b) { return a.entry < b.entry; });
        std::string s;
        bool all_same = true, spread = true;
        for (int w = 0; w < NWV; ++w)
        {
            int seen[4] = {0, 0, 0, 0};
            for (auto &g : v) { seen[g.simd[w]]++; all_same = all_same && g.simd[w] == v[0].simd[w]; }
            for (int i = 0; i < 4; ++i) spread = spread && seen[i] <= 1;
        }
        for (auto &g : v)
        {
            for (int w = 0; w < NWV; ++w) s += char('0' + g.simd[w]);
            s += ' ';
        }
        patterns[s]++;
        ++cus;
        same += all_same && v.size() > 1;
        per_simd_one_each += spread;
        int w0[4] = {0, 0, 0, 0};
        for (auto &g : v) w0[g.simd[0]]++;
        wave0_shared += *std::max_element(w0, w0 + 4) > 1;
    }
    printf("%u channels, %d blocks per launch: %d CUs with workgroups\n", C, K, cus);
    printf("CUs whose workgroups all have the same wave -> SIMD map:              %d\n", same);
    printf("CUs where no pipeline position shares a SIMD between two workgroups: %d\n", per_simd_one_each);
    printf("CUs where the first position (wave 0) of two workgroups shares a SIMD: %d\n", wave0_shared);
    printf("patterns (SIMD of waves 0123 per workgroup, workgroups of a CU in the order of entry) and how many CUs show them:\n");
    std::vector<std::pair<int, std::string>> byn;
    for (auto &kv : patterns) byn.push_back({kv.second, kv.first});
    std::sort(byn.rbegin(), byn.rend());
    for (size_t i = 0; i < byn.size() && i < 24; ++i) printf("  %4d  %s\n", byn[i].first, byn[i].second.c_str());
    printf("the first eight CUs: workgroup (blockIdx.x): SIMD of waves 0 1 2 3\n");
    int shown = 0;
    for (auto &kv : cu)
    {
        if (shown++ == 8) break;
        printf("  xcd %u se %u sh %u cu %2u:", kv.first >> 12, (kv.first >> 8) & 7, (kv.first >> 4) & 1, kv.first & 15);
        for (auto &g : kv.second) printf("  %4u: %d %d %d %d", g.b, g.simd[0], g.simd[1], g.simd[2], g.simd[3]);
        printf("\n");
    }
    return 0;
}
