// quantized_counter_bank.h on the host, without the library and without a device: the bin of a sample and the closed form of one
// call as the kernel and the class compile them, written out for tests/test_quantized_counter_host.py to hold against the numpy
// restatement.
//   quantized_counter_plan IN OUT    IN: float32 samples.  OUT: for each of six ranges and four level counts fRStep and the
//                                    counter word of every sample (nMaxLevels 300), then rows of 13 words: nCapacity, nPeriod,
//                                    nHead, nCount, n and the eight words of make_plan()
#include "quantized_counter_bank.h"
#include <cstdio>
#include <cstring>
#include <vector>
using namespace mi_qcounter;
int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<float> x(1 << 16);
    const size_t n = fread(x.data(), 4, x.size(), f);
    fclose(f);
    const float R[6][2] = {{-1,1},{-0.5f,0.25f},{0.0f,2.4e-38f},{1,-1},{0.3f,0.3f},{-1e30f,1e30f}};
    const uint32_t L[4] = {1,8,16,300};
    FILE *o = fopen(argv[2], "wb");
    for (int r = 0; r < 6; ++r) for (int l = 0; l < 4; ++l) {
        float rs = rstep_of(L[l], R[r][0], R[r][1]);
        fwrite(&rs, 4, 1, o);
        for (size_t i = 0; i < n; ++i) { uint32_t b = bin_of(scaled(x[i], R[r][0], rs), L[l], 300); fwrite(&b, 4, 1, o); }
    }
    const uint32_t caps[2] = {1040, 1072};
    for (int c = 0; c < 2; ++c) for (uint32_t period : {1u, 5u, 40u}) for (uint32_t head : {0u, 1u, 500u, caps[c]-1}) for (uint32_t count : {0u, 1u, 4u, 5u, 40u, 47u, caps[c]})
        for (uint32_t nn : {0u, 1u, 3u, 39u, 40u, 41u, 999u, 1000u, 1039u, 1040u, 1041u, 1072u, 1073u, 5000u, 2147483647u}) {
            plan p = make_plan(head, count, period, caps[c], nn);
            uint32_t w[13] = {caps[c], period, head, count, nn, p.tail, p.evict, p.remain, p.keep_from, p.store_from, p.store_pos, p.head_after, p.count_after};
            fwrite(w, 4, 13, o);
        }
    fclose(o);
    return 0;
}
