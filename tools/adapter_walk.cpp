// adapter_walk.cpp -- the per-lane arithmetic of adapter_points_kernel (drprg_amd/csrc/adapter_piece.h) walked on the CPU, every buffer at
// its exact size, against the rule stated byte by byte.  Meant for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Idrprg_amd/csrc tools/adapter_walk.cpp -o build/adapter_walk && build/adapter_walk
// Random batches of short and long reads, text and packed form, ranges narrower than the reads, one to four adapters of 1..64 letters.
// Exit status 0: every cut equals the rule's.
#include "adapter_piece.h"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

using namespace drprg::dev;

static uint64_t read_holding_host(const uint64_t* offsets, uint64_t lo, uint64_t hi, uint64_t p)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

static bool is_base(uint8_t c) { return ad_letter(c) < 4; }

// the rule, byte by byte
static uint32_t rule_cut(const std::vector<uint8_t>& text, uint64_t x, uint64_t y, const std::vector<std::string>& adapters, uint32_t e, uint32_t O)
{
    const uint64_t n = y - x;
    for (uint64_t p = 0; p < n; ++p)
        for (const std::string& A : adapters) {
            const uint64_t m = A.size(), c = m < n - p ? m : n - p;
            if (c < O) continue;
            uint64_t miss = 0;
            for (uint64_t j = 0; j < c; ++j) {
                const uint8_t b = text[x + p + j];
                if (!is_base(b) || (b & 0xDF) != (A[j] & 0xDF)) ++miss;
            }
            if (miss <= c * e / 1000) return (uint32_t)p;
        }
    return AD_NONE;
}

int main()
{
    std::mt19937_64 rng(20240611);
    auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    const char letters[] = "ACGTacgtN";
    uint64_t checked = 0, cuts = 0;
    for (int round = 0; round < 400; ++round) {
        AdapterSet ad {};
        std::vector<std::string> adapters;
        ad.n = 1 + (uint32_t)rnd(round % 4 == 0 ? 4 : 1);
        uint32_t shortest = 64;
        for (uint32_t a = 0; a < ad.n; ++a) {
            const uint32_t m = round % 7 == 0 ? 1 + (uint32_t)rnd(64) : (uint32_t[]) { 12, 16, 17, 33, 64, 5, 32, 48 }[rnd(8)];
            std::string A;
            for (uint32_t j = 0; j < m; ++j) A += letters[rnd(8)];
            adapters.push_back(A);
            ad.len[a] = m;
            for (uint32_t j = 0; j < m; ++j) (j < 32 ? ad.lo[a] : ad.hi[a]) |= (uint64_t)ad_letter((uint8_t)A[j]) << (2 * (j & 31));
            if (m > ad.max_len) ad.max_len = m;
            if (m < shortest) shortest = m;
        }
        ad.error_milli = (uint32_t[]) { 0, 100, 200, 500, 333 }[rnd(5)];
        ad.min_overlap = 1 + (uint32_t)rnd(shortest < 6 ? shortest : 6);
        // a batch: reads of 0..40 bases and a few long ones, adapters planted whole, partial and with errors
        std::vector<uint64_t> offsets { 0 }, begin, end;
        std::vector<uint8_t> text;
        const uint32_t n_reads = 1 + (uint32_t)rnd(300);
        for (uint32_t i = 0; i < n_reads; ++i) {
            uint64_t L = rnd(10) == 0 ? 200 + rnd(3000) : rnd(41);
            std::string r;
            for (uint64_t j = 0; j < L; ++j) r += letters[rnd(100) == 0 ? 8 : rnd(8)];
            if (L && rnd(2)) { // plant
                const std::string& A = adapters[rnd(adapters.size())];
                std::string B = A;
                for (uint64_t k = rnd(4); k > 0; --k) B[rnd(B.size())] = letters[rnd(9)];
                const uint64_t at = rnd(L);
                for (uint64_t j = 0; j < B.size() && at + j < L; ++j) r[at + j] = B[j];
            }
            text.insert(text.end(), r.begin(), r.end());
            offsets.push_back(text.size());
            uint64_t b = 0, t = L;
            if (rnd(4) == 0 && L) {
                b = rnd(L + 1);
                t = b + rnd(L - b + 1);
            }
            begin.push_back(b);
            end.push_back(t);
        }
        const uint64_t n_bases = text.size();
        if (!n_bases) continue;
        // the packed form: words, bitmap
        const uint64_t n_words = (n_bases + 15) / 16;
        std::vector<uint32_t> words(n_words, 0);
        std::vector<uint16_t> bits(n_words, 0);
        for (uint64_t i = 0; i < n_bases; ++i) {
            words[i >> 4] |= (uint32_t)((text[i] >> 1) & 3u) << (2 * (i & 15));
            if (!is_base(text[i])) bits[i >> 4] |= (uint16_t)(1u << (i & 15));
        }
        for (int form = 0; form < 2; ++form) {
            std::vector<uint32_t> cut(n_reads, AD_NONE);
            auto load = [&](uint64_t p, uint32_t& code, uint32_t& nm) {
                code = 0;
                nm = 0xFFFFu;
                if (p >= n_bases) return;
                if (form) {
                    code = words[p >> 4];
                    nm = bits[p >> 4];
                    return;
                }
                uint32_t w[4] = { 0, 0, 0, 0 };
                for (uint32_t j = 0; j < 16 && p + j < n_bases; ++j) w[j >> 2] |= (uint32_t)text[p + j] << (8 * (j & 3));
                ad_text16(w, code, nm);
            };
            const uint32_t extra = (ad.max_len + 14u) / 16u;
            for (uint64_t p = 0; p < n_bases; p += 16) {
                uint32_t c[AD_LANE_WORDS], n[AD_LANE_WORDS];
                for (uint32_t k = 0; k < AD_LANE_WORDS; ++k) {
                    c[k] = 0;
                    n[k] = 0;
                    if (k <= extra) load(p + 16 * k, c[k], n[k]);
                }
                const AdWindow w = ad_window(c, n);
                uint64_t r = read_holding_host(offsets.data(), 0, n_reads - 1, p);
                const uint32_t nst = (uint32_t)(n_bases - p < 16 ? n_bases - p : 16);
                ad_piece(offsets.data(), begin.data(), end.data(), n_reads, n_bases, p, nst, w, ad, r, n_reads - 1, [&](uint64_t read, uint32_t at) {
                    if (read >= n_reads) abort();
                    if (at < cut[read]) cut[read] = at;
                });
            }
            for (uint32_t i = 0; i < n_reads; ++i) {
                const uint32_t want = end[i] > begin[i] ? rule_cut(text, offsets[i] + begin[i], offsets[i] + end[i], adapters, ad.error_milli, ad.min_overlap) : AD_NONE;
                ++checked;
                if (want != AD_NONE) ++cuts;
                if (want != cut[i]) {
                    std::fprintf(stderr, "round %d form %d read %u: cut %u, the rule says %u\n", round, form, i, cut[i], want);
                    return 1;
                }
            }
        }
    }
    std::printf("adapter_walk: %llu reads checked, %llu with a cut\n", (unsigned long long)checked, (unsigned long long)cuts);
    return cuts ? 0 : 1;
}
