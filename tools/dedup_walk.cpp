// dedup_walk.cpp -- walks the word arithmetic of duplicate removal (csrc/dedup_word.h: what dedup_keys_kernel of csrc/dedup.hip runs per
// 16-base window, and what its exact check reads per word) on the CPU, against a straightforward per-read loop over the bases, with every
// buffer at its exact size so that a sanitizer sees any index that leaves it.  Host only; no device, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idrprg_amd/csrc tools/dedup_walk.cpp -o build/dedup_walk
//   build/dedup_walk [batches] [seed]
#include "dedup_word.h"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

using namespace drprg::dev;

// the rule, base by base: letter[] 0..3, masked[] 0/1
static uint64_t plain_key(const uint8_t* letter, const uint8_t* masked, uint64_t L, std::vector<uint64_t>* xs)
{
    if (!L) return 0;
    uint64_t key = dd_fin(DD_GOLDEN * L);
    for (uint64_t j = 0; 16 * j < L; ++j) {
        uint64_t v = 0, m = 0;
        for (uint64_t t = 0; t < 16 && 16 * j + t < L; ++t) {
            v |= (uint64_t)(masked[16 * j + t] ? 0 : letter[16 * j + t]) << (2 * t);
            m |= (uint64_t)masked[16 * j + t] << t;
        }
        const uint64_t x = v | m << 32;
        if (xs) xs->push_back(x);
        key += dd_fin(x + DD_GOLDEN * (j + 1));
    }
    return key;
}

int main(int argc, char** argv)
{
    const long batches = argc > 1 ? std::atol(argv[1]) : 4000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    auto upto = [&](uint64_t n) { return (uint64_t)(rng() % (n + 1)); };
    uint64_t reads_checked = 0, words_checked = 0, phases[16] = {}, tails[17] = {}, with_mask = 0;
    for (long bt = 0; bt < batches; ++bt) {
        const uint64_t n_reads = 1 + upto(bt % 7 == 0 ? 3 : 60);
        std::vector<uint64_t> off(n_reads + 1, 0);
        for (uint64_t i = 0; i < n_reads; ++i) {
            static const uint64_t pick[] = { 0, 0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 150, 400 };
            const uint64_t len = upto(9) == 0 ? upto(1200) : pick[upto(14)];
            off[i + 1] = off[i] + len;
        }
        const uint64_t n_bases = off[n_reads], n_words = (n_bases + 15) / 16;
        if (!n_bases) continue;
        const bool any_mask = bt % 3 != 0;
        std::vector<uint8_t> letter(n_bases), masked(n_bases, 0);
        for (auto& c : letter) c = (uint8_t)(rng() & 3);
        if (any_mask)
            for (auto& c : masked) c = upto(bt % 2 ? 40 : 3) == 0;
        // exact sizes: a sanitizer sees every index beyond the last word
        std::unique_ptr<uint32_t[]> words(new uint32_t[n_words]());
        std::unique_ptr<uint16_t[]> bits(any_mask ? new uint16_t[n_words]() : nullptr);
        std::unique_ptr<uint64_t[]> d_off(new uint64_t[n_reads + 1]);
        for (uint64_t p = 0; p < n_bases; ++p) {
            words[p >> 4] |= (uint32_t)letter[p] << (2 * (p & 15)); // (a masked base keeps some letter in the packed form: the rule forces it to 0)
            if (masked[p]) bits[p >> 4] |= (uint16_t)(1u << (p & 15));
        }
        for (uint64_t i = 0; i <= n_reads; ++i) d_off[i] = off[i];
        const DedupBatch b { words.get(), bits.get(), d_off.get(), n_reads, n_bases };
        // as the kernel: every window of the batch once, lanes of four windows that start from the read holding their first base
        std::vector<uint64_t> key(n_reads, 0);
        bool bad = false;
        for (uint64_t w0 = 0; w0 < n_words; w0 += 4) {
            uint64_t r = 0;
            while (r + 1 < n_reads && d_off[r + 1] <= (w0 << 4)) ++r;
            for (uint64_t w = w0; w < w0 + 4 && w < n_words; ++w) {
                const uint32_t lo = words[w], hi = w + 1 < n_words ? words[w + 1] : 0;
                const uint32_t mlo = bits ? bits[w] : 0, mhi = bits && w + 1 < n_words ? bits[w + 1] : 0;
                dd_window(b, w << 4, lo, hi, mlo, mhi, r, bad, [&](uint64_t read, uint64_t t) {
                    key[read] += t;
                    ++words_checked;
                });
            }
        }
        if (bad) {
            std::fprintf(stderr, "batch %ld: offsets reported at odds\n", bt);
            return 1;
        }
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint64_t L = off[i + 1] - off[i];
            std::vector<uint64_t> xs;
            const uint64_t want = plain_key(letter.data() + off[i], masked.data() + off[i], L, &xs);
            if (key[i] != want) {
                std::fprintf(stderr, "batch %ld read %llu (start %llu, %llu bases): key %016llx, the per-read loop says %016llx\n", bt, (unsigned long long)i,
                    (unsigned long long)off[i], (unsigned long long)L, (unsigned long long)key[i], (unsigned long long)want);
                return 1;
            }
            for (uint64_t j = 0; j < xs.size(); ++j) // what the exact check reads
                if (dd_read_word(words.get(), bits.get(), off[i], L, j) != xs[j]) {
                    std::fprintf(stderr, "batch %ld read %llu word %llu: dd_read_word differs from the rule\n", bt, (unsigned long long)i, (unsigned long long)j);
                    return 1;
                }
            if (L) {
                ++phases[off[i] & 15];
                ++tails[L % 16 ? L % 16 : 16];
                for (uint64_t p = off[i]; p < off[i + 1]; ++p)
                    if (masked[p]) {
                        ++with_mask;
                        break;
                    }
            }
            ++reads_checked;
        }
    }
    int seen = 0, tail_seen = 0;
    for (int p = 0; p < 16; ++p) seen += phases[p] != 0;
    for (int p = 1; p <= 16; ++p) tail_seen += tails[p] != 0;
    std::printf("dedup_walk: %ld batches, %llu reads (%llu with masked bases), %llu read-aligned words, %d of 16 phases and %d of 16 tail lengths seen: OK\n", batches,
        (unsigned long long)reads_checked, (unsigned long long)with_mask, (unsigned long long)words_checked, seen, tail_seen);
    return seen == 16 && tail_seen == 16 ? 0 : 1;
}
