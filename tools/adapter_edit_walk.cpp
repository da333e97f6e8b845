// adapter_edit_walk.cpp -- the per-lane arithmetic of adapter_edit_points_kernel (drprg_amd/csrc/adapter_edit.h) walked on the CPU, every
// buffer at its exact size, against the indel rule stated as a plain dynamic programme.  Meant for a sanitizer build:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -Idrprg_amd/csrc tools/adapter_edit_walk.cpp -o build/adapter_edit_walk && build/adapter_edit_walk
// Random batches of short and long reads; text that is not aligned (no padding), aligned text (64 bytes of padding) and the packed form;
// ranges narrower than the reads; zero to four adapters of 1..64 letters on either side, planted with substitutions, insertions and
// deletions; the 3' side, then the 5' side on what it left, as launch_adapter_edit runs them.  Every batch is walked twice, in stretches
// of AE_STRETCH bases and in stretches of 7: the cuts must not depend on the geometry.  Exit status 0: every range equals the rule's.
#include "adapter_edit.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace drprg::dev;

static bool is_base(uint8_t c) { return ad_letter(c) < 4; }
static bool same(uint8_t base, uint8_t letter) { return is_base(base) && (base & 0xDF) == (letter & 0xDF); }

// the 3' rule on r[0..n): the smallest matching start, or AD_NONE
static uint32_t rule_cut(const std::vector<uint8_t>& r, const std::vector<std::string>& adapters, uint32_t e, uint32_t O)
{
    const size_t n = r.size();
    std::vector<char> match(n, 0);
    for (const std::string& A : adapters) {
        const size_t m = A.size();
        // full[p] = min over q of ed(A, r[p..q)): the reversed adapter against the reversed read, free start, D[i][j] over i letters and j bases
        std::vector<uint32_t> full(n + 1, (uint32_t)m), col(m + 1), nxt(m + 1);
        for (size_t i = 0; i <= m; ++i) col[i] = (uint32_t)i;
        for (size_t j = 1; j <= n; ++j) {
            const uint8_t b = r[n - j];
            nxt[0] = 0;
            for (size_t i = 1; i <= m; ++i) nxt[i] = std::min({ col[i - 1] + (same(b, (uint8_t)A[m - i]) ? 0u : 1u), col[i] + 1u, nxt[i - 1] + 1u });
            col.swap(nxt);
            full[n - j] = col[m];
        }
        for (size_t p = 0; p < n; ++p) {
            const size_t c = n - p;
            if (full[p] <= m * e / 1000 && full[p + 1] >= full[p]) match[p] = 1;
            if (c < m && c >= O) {
                size_t miss = 0;
                for (size_t j = 0; j < c; ++j) miss += same(r[p + j], (uint8_t)A[j]) ? 0 : 1;
                if (miss <= c * e / 1000) match[p] = 1;
            }
        }
    }
    for (size_t p = 0; p < n; ++p)
        if (match[p]) return (uint32_t)p;
    return AD_NONE;
}

static AdapterSet make_set(const std::vector<std::string>& adapters, uint32_t e, uint32_t O)
{
    AdapterSet ad {};
    ad.n = (uint32_t)adapters.size();
    for (uint32_t a = 0; a < ad.n; ++a) {
        const std::string& A = adapters[a];
        ad.len[a] = (uint32_t)A.size();
        for (uint32_t j = 0; j < A.size(); ++j) (j < 32 ? ad.lo[a] : ad.hi[a]) |= (uint64_t)ad_letter((uint8_t)A[j]) << (2 * (j & 31));
        ad.max_len = std::max(ad.max_len, ad.len[a]);
    }
    if (ad.n) {
        ad.error_milli = e;
        ad.min_overlap = O;
    }
    return ad;
}

int main()
{
    std::mt19937_64 rng(20241019);
    auto rnd = [&](uint64_t n) { return (uint64_t)(rng() % n); };
    const char letters[] = "ACGTacgtN";
    uint64_t checked = 0, cuts3 = 0, cuts5 = 0;
    for (int round = 0; round < 240; ++round) {
        std::vector<std::string> ad3s, ad5s;
        const uint32_t n3 = (uint32_t)rnd(round % 4 == 0 ? 5 : 2), n5 = n3 == 0 ? 1 + (uint32_t)rnd(2) : (uint32_t)rnd(round % 3 == 0 ? 5 : 2);
        uint32_t shortest = 64;
        const bool narrow = round % 2 == 0; // every adapter of at most 32 letters: the 32-bit form
        auto draw = [&](std::vector<std::string>& to, uint32_t n) {
            for (uint32_t a = 0; a < n; ++a) {
                uint32_t m = round % 7 == 0 ? 1 + (uint32_t)rnd(64) : (uint32_t[]) { 12, 16, 17, 33, 64, 5, 32, 48 }[rnd(8)];
                if (narrow && m > 32) m -= 32;
                std::string A;
                for (uint32_t j = 0; j < m; ++j) A += letters[rnd(8)];
                to.push_back(A);
                shortest = std::min(shortest, m);
            }
        };
        draw(ad3s, n3);
        draw(ad5s, n5);
        const uint32_t e = (uint32_t[]) { 0, 100, 200, 500, 333 }[rnd(5)], O = 1 + (uint32_t)rnd(shortest < 6 ? shortest : 6);
        std::vector<std::string> ad5r = ad5s;
        for (std::string& A : ad5r) std::reverse(A.begin(), A.end());
        const AdapterSet set3 = make_set(ad3s, e, O), set5 = ae_reversed(make_set(ad5s, e, O));
        {
            const AdapterSet direct = make_set(ad5r, e, O);
            if (std::memcmp(&direct, &set5, sizeof direct) != 0) {
                std::fprintf(stderr, "round %d: ae_reversed is not the set of the reversed adapters\n", round);
                return 1;
            }
        }
        const AdapterEq eq3 = ae_make_eq(set3), eq5 = ae_make_eq(set5);
        // a batch: reads of 0..40 bases and a few long ones, adapters planted whole, cut short and with edits of every kind
        std::vector<uint64_t> offsets { 0 }, begin, end;
        std::vector<uint8_t> text;
        const uint32_t n_reads = 1 + (uint32_t)rnd(200);
        auto edited = [&](std::string B) {
            for (uint64_t k = rnd(5); k > 0 && !B.empty(); --k) {
                const uint64_t at = rnd(B.size()), kind = rnd(3);
                if (kind == 0) B[at] = letters[rnd(9)];
                else if (kind == 1) B.insert(B.begin() + (long)at, letters[rnd(8)]);
                else B.erase(B.begin() + (long)at);
            }
            return B;
        };
        for (uint32_t i = 0; i < n_reads; ++i) {
            uint64_t L = rnd(10) == 0 ? 200 + rnd(1500) : rnd(41);
            std::string r;
            for (uint64_t j = 0; j < L; ++j) r += letters[rnd(100) == 0 ? 8 : rnd(8)];
            if (L && !ad3s.empty() && rnd(2)) {
                const std::string B = edited(ad3s[rnd(ad3s.size())]);
                const uint64_t at = rnd(L);
                r = r.substr(0, at) + B + (rnd(2) ? r.substr(at) : std::string());
            }
            if (!ad5s.empty() && rnd(2)) {
                const std::string B = edited(ad5s[rnd(ad5s.size())]);
                r = (rnd(2) ? r.substr(0, rnd(6)) : std::string()) + B.substr(rnd(3) ? 0 : rnd(B.size() + 1)) + r;
            }
            L = r.size();
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
        // the rule: the 3' cut, then the 5' cut on what is left
        std::vector<uint64_t> want_b = begin, want_e = end;
        for (uint32_t i = 0; i < n_reads; ++i) {
            if (want_e[i] > want_b[i] && !ad3s.empty()) {
                const std::vector<uint8_t> r(text.begin() + (long)(offsets[i] + want_b[i]), text.begin() + (long)(offsets[i] + want_e[i]));
                const uint32_t p = rule_cut(r, ad3s, e, O);
                if (p != AD_NONE) {
                    want_e[i] = want_b[i] + p;
                    ++cuts3;
                }
            }
            if (want_e[i] > want_b[i] && !ad5s.empty()) {
                std::vector<uint8_t> r(text.begin() + (long)(offsets[i] + want_b[i]), text.begin() + (long)(offsets[i] + want_e[i]));
                std::reverse(r.begin(), r.end());
                const uint32_t p = rule_cut(r, ad5r, e, O);
                if (p != AD_NONE) {
                    want_b[i] += r.size() - p;
                    ++cuts5;
                }
            }
        }
        // the three forms, every buffer at its exact size
        const uint64_t n_words = (n_bases + 15) / 16;
        std::vector<uint32_t> words(n_words, 0);
        std::vector<uint16_t> bits(n_words, 0);
        for (uint64_t i = 0; i < n_bases; ++i) {
            words[i >> 4] |= (uint32_t)((text[i] >> 1) & 3u) << (2 * (i & 15));
            if (!is_base(text[i])) bits[i >> 4] |= (uint16_t)(1u << (i & 15));
        }
        std::vector<uint8_t> exact(n_bases + 1);
        uint8_t* const unaligned = exact.data() + 1; // ends where the allocation ends; ae_scan is told that it is not aligned
        std::memcpy(unaligned, text.data(), n_bases);
        void* al = nullptr;
        if (posix_memalign(&al, 16, n_bases + 64)) return 1;
        std::memcpy(al, text.data(), n_bases);
        std::memset((uint8_t*)al + n_bases, 'A', 64); // (padding that would match an adapter if it were looked at as bases)
        for (int form = 0; form < 3; ++form)
            for (uint64_t stretch : { (uint64_t)AE_STRETCH, (uint64_t)7 }) {
                AeBases bs {};
                bs.n_bases = n_bases;
                if (form == 0) bs.text = unaligned;
                if (form == 1) { bs.text = (const uint8_t*)al; bs.aligned = true; }
                if (form == 2) { bs.words = words.data(); bs.nbits = bits.data(); }
                std::vector<uint64_t> b = begin, t = end;
                std::vector<uint32_t> cut(n_reads, AD_NONE);
                const bool wide3 = set3.max_len > 32, wide5 = set5.max_len > 32;
                if (set3.n) {
                    auto emit = [&](uint64_t read, uint32_t v) {
                        if (read >= n_reads) abort();
                        cut[read] = std::min(cut[read], v);
                    };
                    for (uint64_t p = 0; p < n_bases; p += stretch) {
                        const uint64_t to = std::min(p + stretch, n_bases);
                        if (wide3) ae_scan<-1, uint64_t>(bs, offsets.data(), b.data(), t.data(), n_reads, p, to, set3, eq3, emit);
                        else ae_scan<-1, uint32_t>(bs, offsets.data(), b.data(), t.data(), n_reads, p, to, set3, eq3, emit);
                    }
                    for (uint32_t i = 0; i < n_reads; ++i)
                        if (cut[i] != AD_NONE && cut[i] < t[i] - b[i]) t[i] = b[i] + cut[i];
                }
                if (set5.n) {
                    std::fill(cut.begin(), cut.end(), 0u);
                    auto emit = [&](uint64_t read, uint32_t v) {
                        if (read >= n_reads) abort();
                        cut[read] = std::max(cut[read], v);
                    };
                    for (uint64_t p = 0; p < n_bases; p += stretch) {
                        const uint64_t to = std::min(p + stretch, n_bases);
                        if (wide5) ae_scan<1, uint64_t>(bs, offsets.data(), b.data(), t.data(), n_reads, p, to, set5, eq5, emit);
                        else ae_scan<1, uint32_t>(bs, offsets.data(), b.data(), t.data(), n_reads, p, to, set5, eq5, emit);
                    }
                    for (uint32_t i = 0; i < n_reads; ++i)
                        if (cut[i] != 0 && cut[i] <= t[i] - b[i]) b[i] += cut[i];
                }
                for (uint32_t i = 0; i < n_reads; ++i) {
                    ++checked;
                    if (b[i] != want_b[i] || t[i] != want_e[i]) {
                        std::fprintf(stderr, "round %d form %d stretch %llu read %u: [%llu, %llu), the rule says [%llu, %llu) of [%llu, %llu)\n", round, form,
                            (unsigned long long)stretch, i, (unsigned long long)b[i], (unsigned long long)t[i], (unsigned long long)want_b[i],
                            (unsigned long long)want_e[i], (unsigned long long)begin[i], (unsigned long long)end[i]);
                        return 1;
                    }
                }
            }
        std::free(al);
    }
    std::printf("adapter_edit_walk: %llu ranges checked, %llu 3' cuts and %llu 5' cuts by the rule\n", (unsigned long long)checked, (unsigned long long)cuts3,
        (unsigned long long)cuts5);
    return cuts3 && cuts5 ? 0 : 1;
}
