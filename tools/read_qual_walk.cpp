// read_qual_walk.cpp -- walks the index arithmetic of read_qual_kernel (csrc/read_qual.hip) on the CPU: which read a lane's bytes belong to and
// how its 16 bytes are cut into pieces (csrc/read_qual_piece.h: rq_piece, what the kernel runs per lane and round), tile by tile, round by
// round and lane by lane as the kernel visits them, against the rule stated read by read -- with every buffer at its exact size, so that a
// sanitizer sees any index that leaves it.  The threshold T and the keep test are checked beside the sums.  Host only; no device, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Idrprg_amd/csrc tools/read_qual_walk.cpp -o build/read_qual_walk
//   build/read_qual_walk [batches] [seed]
#include "read_qual_piece.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <vector>

using namespace drprg::dev;

namespace {
constexpr uint64_t THREADS = 256, ROUNDS = 4, LANE_BYTES = 16, TILE = THREADS * ROUNDS * LANE_BYTES; // as read_qual.hip
// search.h needs the HIP headers, so its two searches are restated here: read_holding word for word, and what the kernel makes of
// first_at_least for a tile's first and last byte (the wave-wide search itself runs on the device only: tests/test_gpu_read_filter.py
// holds it, with runs of empty reads on a tile edge)
// the kernel's derivation: the first read that starts behind `at`, minus one (0 when there is none before it)
uint64_t tile_read(const uint64_t* offsets, uint64_t n_reads, uint64_t at)
{
    const uint64_t i = (uint64_t)(std::lower_bound(offsets, offsets + n_reads, at + 1) - offsets); // first_at_least(offsets, n_reads, at + 1)
    return i ? i - 1 : 0;
}
// read_holding of search.h: the largest r in [lo, hi] with offsets[r] <= p
uint64_t read_holding(const uint64_t* offsets, uint64_t lo, uint64_t hi, uint64_t p)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (offsets[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
}

int main(int argc, char** argv)
{
    const long batches = argc > 1 ? std::atol(argv[1]) : 3000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    auto upto = [&](uint64_t n) { return (uint64_t)(rng() % (n + 1)); };
    uint64_t reads_checked = 0, pieces = 0, split_pieces = 0, multi_tile_reads = 0, kept = 0;
    long walked = 0;
    for (long b = 0; b < batches; ++b) {
        // reads of mixed lengths: runs of empty reads, lengths around the lane's 16 bytes and the tile, a long read now and then
        const uint64_t n_reads = 1 + upto(b % 7 == 0 ? 3 : 80);
        std::unique_ptr<uint64_t[]> off(new uint64_t[n_reads + 1]); // exact size
        off[0] = 0;
        for (uint64_t i = 0; i < n_reads; ++i) {
            static const uint64_t pick[] = { 0, 0, 0, 1, 2, 15, 16, 17, 31, 32, 33, 150, 400, 4095, 4096, 4097 };
            uint64_t len = pick[upto(15)];
            if (upto(11) == 0) len = upto(3000);
            if (upto(40) == 0) len = TILE - 1 + upto(2);
            if (upto(90) == 0) len = 2 * TILE + upto(3 * TILE);
            off[i + 1] = off[i] + len;
        }
        const uint64_t n_bases = off[n_reads];
        if (!n_bases) continue;
        const uint32_t bias = b & 1 ? 33 : 0;
        std::unique_ptr<uint8_t[]> qual(new uint8_t[n_bases]); // exact size (the kernel's 16-byte loads read the padding; the walk takes n bytes)
        const uint32_t lo_q = (uint32_t)upto(40), span = 1 + (uint32_t)upto(RQ_MAX_QUAL - lo_q);
        for (uint64_t p = 0; p < n_bases; ++p) qual[p] = (uint8_t)(bias + lo_q + upto(span - 1));
        if (upto(3) == 0) qual[upto(n_bases - 1)] = (uint8_t)(bias + 0);
        if (upto(3) == 0) qual[upto(n_bases - 1)] = (uint8_t)(bias + RQ_MAX_QUAL);
        std::vector<uint64_t> want(n_reads, 0), got(n_reads, 0);
        for (uint64_t i = 0; i < n_reads; ++i) {
            for (uint64_t p = off[i]; p < off[i + 1]; ++p) want[i] += RQ_E[qual[p] - bias];
            if (off[i + 1] - off[i] > TILE) ++multi_tile_reads;
        }
        ++walked;
        for (uint64_t tile = 0; tile < n_bases; tile += TILE) {
            const uint64_t tile_end = n_bases - tile > TILE ? tile + TILE : n_bases;
            const uint64_t first = tile_read(off.get(), n_reads, tile), last = tile_read(off.get(), n_reads, tile_end - 1);
            if (first != read_holding(off.get(), 0, n_reads - 1, tile) || last != read_holding(off.get(), 0, n_reads - 1, tile_end - 1)) {
                std::fprintf(stderr, "batch %ld: the two searches disagree on the reads of the tile at %llu\n", b, (unsigned long long)tile);
                return 1;
            }
            for (uint64_t round = 0; round < ROUNDS; ++round)
                for (uint64_t t = 0; t < THREADS; ++t) {
                    const uint64_t p = tile + (round * THREADS + t) * LANE_BYTES;
                    if (p >= tile_end) continue;
                    const uint32_t n = (uint32_t)(tile_end - p < LANE_BYTES ? tile_end - p : LANE_BYTES);
                    uint32_t e[16] = {};
                    for (uint32_t j = 0; j < n; ++j) e[j] = RQ_E[qual[p + j] - bias];
                    uint64_t r = read_holding(off.get(), first, last, p), head = ~0ull;
                    bool split = false;
                    const uint64_t s = rq_piece(off.get(), n_reads, p, n, e, r, head, [&](uint64_t read, uint64_t v) {
                        if (read < first || read > last || read >= n_reads) {
                            std::fprintf(stderr, "batch %ld: a piece for read %llu outside the tile's reads\n", b, (unsigned long long)read);
                            std::exit(1);
                        }
                        got[read] += v;
                        split = true;
                    });
                    if (head < first || head > last) {
                        std::fprintf(stderr, "batch %ld: head read %llu outside the tile's reads\n", b, (unsigned long long)head);
                        return 1;
                    }
                    got[head] += s;
                    ++pieces;
                    split_pieces += split;
                }
        }
        const uint32_t milli = b % 3 == 0 ? (uint32_t)(1000 * (1 + upto(40))) : (uint32_t)(1 + upto(RQ_MAX_QUAL_MILLI - 1));
        const uint64_t T = rq_threshold(milli);
        if (milli % 1000 == 0 && T != RQ_E[milli / 1000]) return 1;
        if (T > RQ_E[milli / 1000] || T < RQ_E[milli / 1000 + (milli % 1000 ? 1 : 0)]) {
            std::fprintf(stderr, "T of %u outside its neighbours in the table\n", milli);
            return 1;
        }
        for (uint64_t i = 0; i < n_reads; ++i) {
            if (got[i] != want[i]) {
                std::fprintf(stderr, "batch %ld read %llu: got %llu want %llu\n", b, (unsigned long long)i, (unsigned long long)got[i], (unsigned long long)want[i]);
                return 1;
            }
            kept += got[i] <= (off[i + 1] - off[i]) * T;
            ++reads_checked;
        }
    }
    std::printf("read_qual_walk: %ld batches, %llu reads (%llu longer than a tile, %llu kept by their batch's threshold), %llu pieces (%llu cut by a read "
                "boundary): OK\n", walked, (unsigned long long)reads_checked, (unsigned long long)multi_tile_reads, (unsigned long long)kept,
        (unsigned long long)pieces, (unsigned long long)split_pieces);
    return split_pieces && multi_tile_reads ? 0 : 1;
}
