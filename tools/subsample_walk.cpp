// subsample_walk.cpp -- walks the word assembly of the packed compaction (csrc/subsample_word.h: what ss_pack_kernel of csrc/subsample.hip
// runs per output word) on the CPU, against a base-by-base statement, with every buffer at its exact size so that a sanitizer sees any
// index that leaves it.  Host only; no device, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idrprg_amd/csrc tools/subsample_walk.cpp -o build/subsample_walk
//   build/subsample_walk [batches] [seed]
#include "subsample_word.h"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

using drprg::dev::CompactBatch;

int main(int argc, char** argv)
{
    const long batches = argc > 1 ? std::atol(argv[1]) : 4000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    auto upto = [&](uint64_t n) { return (uint64_t)(rng() % (n + 1)); };
    uint64_t words_checked = 0, stitched = 0, phases[16] = {};
    long walked = 0;
    for (long b = 0; b < batches; ++b) {
        // an old batch of reads of mixed lengths (runs of empty reads, lengths around the word size, a long read now and then)
        const uint64_t n_old = 1 + upto(b % 7 == 0 ? 3 : 60);
        std::vector<uint64_t> off(n_old + 1, 0);
        for (uint64_t i = 0; i < n_old; ++i) {
            static const uint64_t pick[] = { 0, 0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 150, 400 };
            const uint64_t len = upto(9) == 0 ? upto(1200) : pick[upto(14)];
            off[i + 1] = off[i] + len;
        }
        const uint64_t src_bases = off[n_old], src_nwords = (src_bases + 15) / 16;
        std::vector<uint8_t> base(src_bases);
        for (auto& c : base) c = (uint8_t)(rng() & 3);
        std::unique_ptr<uint32_t[]> src(new uint32_t[src_nwords]()); // exact size
        for (uint64_t p = 0; p < src_bases; ++p) src[p >> 4] |= (uint32_t)base[p] << (2 * (p & 15));
        // the kept reads
        std::vector<uint64_t> new_off { 0 }, start;
        std::vector<uint8_t> want;
        const uint64_t keep_of = 1 + upto(3);
        for (uint64_t i = 0; i < n_old; ++i) {
            if (upto(keep_of) == 0 && b % 5 != 0) continue;
            start.push_back(off[i]);
            want.insert(want.end(), base.begin() + off[i], base.begin() + off[i + 1]);
            new_off.push_back(want.size());
        }
        if (start.empty() || want.empty()) continue;
        std::unique_ptr<uint64_t[]> d_off(new uint64_t[new_off.size()]), d_start(new uint64_t[start.size()]);
        for (size_t i = 0; i < new_off.size(); ++i) d_off[i] = new_off[i];
        for (size_t i = 0; i < start.size(); ++i) d_start[i] = start[i];
        const CompactBatch cb { src.get(), src_bases, d_off.get(), d_start.get(), (uint64_t)start.size(), (uint64_t)want.size() };
        const uint64_t n_words = (want.size() + 15) / 16;
        ++walked;
        // as the kernel: a lane starts at some word with the read that holds its first base and walks on through four words
        for (uint64_t w0 = 0; w0 < n_words; w0 += 4) {
            uint64_t r = 0; // (read_holding's answer: the largest r with new_offsets[r] <= p)
            while (r + 1 < cb.n_reads && d_off[r + 1] <= (w0 << 4)) ++r;
            for (uint64_t w = w0; w < w0 + 4 && w < n_words; ++w) {
                bool bad = false;
                const uint32_t got = drprg::dev::ss_word(cb, w << 4, r, bad);
                uint32_t expect = 0;
                for (uint64_t i = 0; i < 16 && (w << 4) + i < want.size(); ++i) expect |= (uint32_t)want[(w << 4) + i] << (2 * i);
                if (bad || got != expect) {
                    std::fprintf(stderr, "batch %ld word %llu: got %08x want %08x bad %d\n", b, (unsigned long long)w, got, expect, (int)bad);
                    return 1;
                }
                ++words_checked;
                const uint64_t s0 = d_off[r], e0 = d_off[r + 1];
                if (s0 <= (w << 4) && (w << 4) + 16 <= e0) ++phases[(d_start[r] + ((w << 4) - s0)) & 15];
                else ++stitched;
            }
        }
    }
    int seen = 0;
    for (int p = 0; p < 16; ++p) seen += phases[p] != 0;
    std::printf("subsample_walk: %ld batches, %llu words (%llu stitched across a read boundary or the batch's end), %d of 16 source phases seen: OK\n", walked,
        (unsigned long long)words_checked, (unsigned long long)stitched, seen);
    return seen == 16 ? 0 : 1;
}
