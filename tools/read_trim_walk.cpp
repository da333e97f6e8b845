// read_trim_walk.cpp -- walks the index arithmetic of trim_points_kernel and trim_tables_kernel (csrc/read_trim.hip) on the CPU: the 48
// bytes a lane assembles, its 16 window sums, how its starts are cut by read and held against each read's cropped range
// (csrc/read_trim_piece.h: rt_good_bits, rt_piece, rt_crop, rt_range -- what the kernels run per lane and per read), tile by tile, round by
// round and lane by lane as the kernel visits them, against the rule stated read by read -- with every buffer at its exact size plus the
// documented 64 bytes behind the quality bytes, so that a sanitizer sees any index that leaves it.  Host only; no device, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idrprg_amd/csrc tools/read_trim_walk.cpp -o build/read_trim_walk
//   build/read_trim_walk [batches] [seed]
#include "read_trim_piece.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

using namespace drprg::dev;

namespace {
constexpr uint64_t THREADS = 256, ROUNDS = 4, TILE = THREADS * ROUNDS * RT_LANE_STARTS; // as read_trim.hip
// search.h needs the HIP headers: its searches are restated here, as tools/read_qual_walk.cpp restates them
uint64_t tile_read(const uint64_t* offsets, uint64_t n_reads, uint64_t at)
{
    const uint64_t i = (uint64_t)(std::lower_bound(offsets, offsets + n_reads, at + 1) - offsets); // first_at_least(offsets, n_reads, at + 1)
    return i ? i - 1 : 0;
}
uint64_t read_holding(const uint64_t* offsets, uint64_t lo, uint64_t hi, uint64_t p)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the rule, read by read, in READ orientation (include/drprg_hip.h "read trimming"); q: the read's Phred values in read orientation
void rule(const std::vector<uint32_t>& q, uint64_t front, uint64_t tail, uint32_t milli, uint32_t W, uint64_t& a, uint64_t& b)
{
    const uint64_t L = q.size();
    const uint64_t a0 = std::min(front, L), b0 = L - std::min(tail, L - a0);
    a = b = 0;
    if (!milli) {
        if (a0 < b0) a = a0, b = b0;
        return;
    }
    bool any = false;
    uint64_t first = 0, last = 0;
    for (uint64_t i = a0; i + W <= b0; ++i) {
        uint64_t s = 0;
        for (uint32_t j = 0; j < W; ++j) s += q[i + j];
        if (1000 * s >= (uint64_t)milli * W) {
            if (!any) first = i;
            last = i;
            any = true;
        }
    }
    if (!any) return;
    uint64_t x = first, y = last + W;
    while (x < y && 1000 * q[x] < milli) ++x;
    while (y > x && 1000 * q[y - 1] < milli) --y;
    if (x < y) a = x, b = y;
}
}

int main(int argc, char** argv)
{
    const long batches = argc > 1 ? std::atol(argv[1]) : 1500;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    auto upto = [&](uint64_t n) { return (uint64_t)(rng() % (n + 1)); };
    uint64_t reads_checked = 0, pieces = 0, emits = 0, multi_tile_reads = 0, cls[5] = { 0, 0, 0, 0, 0 }; // untouched, front, tail, both, emptied
    long walked = 0;
    // the four-bytes-at-once range test against the test byte by byte: every byte value at every place, both biases
    for (uint32_t bias : { 0u, 33u })
        for (uint32_t v = 0; v < 256; ++v)
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t fill = bias + (uint32_t)upto(RT_MAX_QUAL), x = (fill * 0x01010101u & ~(0xFFu << (8 * k))) | (v << (8 * k));
                const bool bad = v < bias || v > bias + RT_MAX_QUAL;
                if (rt_bad_bytes(x, bias) != (bad ? 0x80u << (8 * k) : 0u)) {
                    std::fprintf(stderr, "rt_bad_bytes: byte %u at place %u under bias %u\n", v, k, bias);
                    return 1;
                }
            }
    for (long bno = 0; bno < batches; ++bno) {
        const uint64_t n_reads = 1 + upto(bno % 7 == 0 ? 3 : 80);
        std::unique_ptr<uint64_t[]> off(new uint64_t[n_reads + 1]); // exact size
        std::unique_ptr<uint8_t[]> rev(new uint8_t[n_reads]);
        off[0] = 0;
        for (uint64_t i = 0; i < n_reads; ++i) {
            static const uint64_t pick[] = { 0, 0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 150, 400, 4097 };
            uint64_t len = pick[upto(15)];
            if (upto(11) == 0) len = upto(3000);
            if (upto(40) == 0) len = TILE - 1 + upto(2);
            if (upto(90) == 0) len = 2 * TILE + upto(3 * TILE);
            off[i + 1] = off[i] + len;
            rev[i] = upto(2) == 0;
        }
        const uint64_t n_bases = off[n_reads];
        if (!n_bases) continue;
        const uint32_t bias = bno & 1 ? 33 : 0;
        const uint32_t W = bno % 5 == 0 ? 1 : (bno % 5 == 1 ? 32 : (bno % 5 == 2 ? 4 : 1 + (uint32_t)upto(31)));
        const uint32_t milli = bno % 3 == 0 ? (uint32_t)(1000 * (1 + upto(40))) : (uint32_t)(1 + upto(RT_MAX_QUAL_MILLI - 1));
        const uint64_t front = upto(3) == 0 ? upto(20) : 0, tail = upto(3) == 0 ? upto(20) : 0;
        std::unique_ptr<uint8_t[]> qual(new uint8_t[n_bases + 64]); // the documented size: n_bases and 64 zero bytes
        std::memset(qual.get() + n_bases, 0, 64);
        // runs of good and bad bytes around the threshold, so that windows are good in places
        const uint32_t Q = milli / 1000;
        for (uint64_t p = 0; p < n_bases;) {
            const uint64_t run = 1 + upto(upto(3) ? 40 : 2000);
            const bool good = upto(1);
            for (uint64_t j = 0; j < run && p < n_bases; ++j, ++p) {
                const uint32_t lo = good ? std::min(Q, RT_MAX_QUAL) : 0, hi = good ? RT_MAX_QUAL : std::min(Q + 1, RT_MAX_QUAL);
                qual[p] = (uint8_t)(bias + lo + upto(hi - lo));
            }
        }
        const uint32_t thr = rt_window_threshold(milli, bias, W);
        std::vector<uint32_t> gmin(n_reads, RT_NONE), gmax(n_reads, 0);
        ++walked;
        for (uint64_t tile = 0; tile < n_bases; tile += TILE) {
            const uint64_t tile_end = n_bases - tile > TILE ? tile + TILE : n_bases;
            const uint64_t first = tile_read(off.get(), n_reads, tile), last = tile_read(off.get(), n_reads, tile_end - 1);
            for (uint64_t round = 0; round < ROUNDS; ++round)
                for (uint64_t t = 0; t < THREADS; ++t) {
                    const uint64_t p = tile + (round * THREADS + t) * RT_LANE_STARTS;
                    if (p >= tile_end) continue;
                    const uint32_t n = (uint32_t)(tile_end - p < RT_LANE_STARTS ? tile_end - p : RT_LANE_STARTS);
                    // the lane's own 16 bytes and -- W > 1 / W > 17 -- the one or two 16-byte pieces behind them, as the kernel loads them
                    // (every load starts below n_bases + 48 and ends inside the padding)
                    uint32_t w[RT_LANE_WORDS] = {};
                    const uint32_t loads = 1 + (W > 1) + (W > 17);
                    for (uint32_t l = 0; l < loads; ++l) {
                        if (l && p + 16 * l >= n_bases + 48) return 1; // (cannot be: p < n_bases)
                        std::memcpy(w + 4 * l, qual.get() + p + 16 * l, 16);
                    }
                    const uint32_t good = rt_good_bits(w, W, thr);
                    uint64_t r = read_holding(off.get(), first, last, p);
                    rt_piece(off.get(), rev.get(), n_reads, n_bases, p, n, good, W, front, tail, r, [&](uint64_t read, uint32_t f, uint32_t l1) {
                        if (read < first || read > last || read >= n_reads) {
                            std::fprintf(stderr, "batch %ld: a piece for read %llu outside the tile's reads\n", bno, (unsigned long long)read);
                            std::exit(1);
                        }
                        gmin[read] = std::min(gmin[read], f);
                        gmax[read] = std::max(gmax[read], l1);
                        ++emits;
                    });
                    ++pieces;
                }
        }
        // trim_tables_kernel, read by read, against the rule in read orientation
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint64_t s = off[i], L = off[i + 1] - off[i];
            uint64_t lo, hi, p, q;
            rt_crop(L, front, tail, rev[i], lo, hi);
            rt_range(qual.get() + s, lo, hi, gmin[i], gmax[i], W, bias, milli, p, q);
            const uint64_t x = rev[i] ? (q > p ? L - q : 0) : p, y = rev[i] ? (q > p ? L - p : 0) : q;
            std::vector<uint32_t> ro(L);
            for (uint64_t j = 0; j < L; ++j) ro[j] = qual[s + (rev[i] ? L - 1 - j : j)] - bias;
            uint64_t a, b;
            rule(ro, front, tail, milli, W, a, b);
            if (a != x || b != y) {
                std::fprintf(stderr, "batch %ld read %llu (L %llu, rev %d, W %u, Q %u, crops %llu/%llu): got [%llu, %llu) want [%llu, %llu)\n", bno,
                    (unsigned long long)i, (unsigned long long)L, (int)rev[i], W, milli, (unsigned long long)front, (unsigned long long)tail,
                    (unsigned long long)x, (unsigned long long)y, (unsigned long long)a, (unsigned long long)b);
                return 1;
            }
            if (L > TILE) ++multi_tile_reads;
            if (L) ++cls[a == b ? 4 : (a == 0 && b == L ? 0 : (a > 0 && b < L ? 3 : (a > 0 ? 1 : 2)))];
            ++reads_checked;
        }
        // the crops alone (no quality): the range is the crop
        for (uint64_t i = 0; i < n_reads; ++i) {
            const uint64_t L = off[i + 1] - off[i];
            uint64_t lo, hi, a, b;
            rt_crop(L, front, tail, rev[i], lo, hi);
            rule(std::vector<uint32_t>(L, 0), front, tail, 0, 0, a, b);
            const uint64_t x = lo < hi ? (rev[i] ? L - hi : lo) : 0, y = lo < hi ? (rev[i] ? L - lo : hi) : 0;
            if (a != x || b != y) return 1;
        }
    }
    std::printf("read_trim_walk: %ld batches, %llu reads (%llu longer than a tile; untouched %llu, front %llu, tail %llu, both %llu, emptied %llu), %llu pieces, "
                "%llu (piece, read) pairs with a good window: OK\n", walked, (unsigned long long)reads_checked, (unsigned long long)multi_tile_reads,
        (unsigned long long)cls[0], (unsigned long long)cls[1], (unsigned long long)cls[2], (unsigned long long)cls[3], (unsigned long long)cls[4],
        (unsigned long long)pieces, (unsigned long long)emits);
    return multi_tile_reads && cls[0] && cls[1] && cls[2] && cls[3] && cls[4] ? 0 : 1;
}
