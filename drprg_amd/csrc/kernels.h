// kernels.h -- argument blocks and launch wrappers of kernels.hip (host side sees only hip_runtime_api).
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime_api.h>
#include "switches.h"

#if defined(__HIPCC__)
#define DRPRG_HD __host__ __device__
#else
#define DRPRG_HD
#endif
#include "dedup_word.h"
#include "adapter_piece.h"
#include "adapter_edit.h"
#include "decoy_piece.h"
#include "poly_piece.h"
#include "read_stats_words.h"

namespace drprg {
namespace dev {

// hit sort key: [read:28][prg:12][rev:1][pos:23]; forward hits (rev=0) sort first
constexpr int HIT_POS_BITS = 23;
constexpr int HIT_PRG_BITS = 12;
constexpr int HIT_READ_BITS = 28;
constexpr uint64_t HIT_POS_MASK = (1ull << HIT_POS_BITS) - 1;
constexpr uint32_t MAX_BATCH_READS = 1u << HIT_READ_BITS;
constexpr uint32_t MAX_PRGS = 1u << HIT_PRG_BITS;

DRPRG_HD inline uint64_t pack_hit_key(uint32_t read, uint32_t prg, uint32_t rev, uint32_t pos)
{
    return ((uint64_t)read << (HIT_PRG_BITS + 1 + HIT_POS_BITS)) | ((uint64_t)prg << (1 + HIT_POS_BITS))
        | ((uint64_t)rev << HIT_POS_BITS) | (uint64_t)pos;
}
DRPRG_HD inline uint32_t hit_read(uint64_t k) { return (uint32_t)(k >> (HIT_PRG_BITS + 1 + HIT_POS_BITS)); }
DRPRG_HD inline uint32_t hit_prg(uint64_t k) { return (uint32_t)(k >> (1 + HIT_POS_BITS)) & (MAX_PRGS - 1); }
DRPRG_HD inline uint32_t hit_rev(uint64_t k) { return (uint32_t)(k >> HIT_POS_BITS) & 1u; }

// Bloom tier in front of the hash table (direct kernel, large indexes): word and two bits from one multiplicative hash
DRPRG_HD inline uint32_t pbloom_mix(uint64_t key) { return ((uint32_t)key ^ (uint32_t)(key >> 32)) * 0x9E3779B1u; }
DRPRG_HD inline uint32_t pbloom_word(uint32_t m, uint32_t wbits) { return m >> (32 - wbits); }
DRPRG_HD inline uint32_t pbloom_bits(uint32_t m) { return (1u << (m & 31)) | (1u << ((m >> 5) & 31)); }

struct SketchArgs {
    const uint8_t* bases;    // 16-byte aligned.  packed != 0: the same pointer is u32 words[ceil(n_bases / 16)], 2 bits per base
    const uint64_t* offsets; // n_reads + 1 (in bases, whatever the format)
    uint64_t n_bases;
    uint32_t n_reads;
    int w, k, halo;
    // 2-bit packed reads (SURVEY.md section 8f NEXT-4; include/drprg_hip.h "packed reads"): base i of the batch is bits
    // [2 (i & 15) + 1 : 2 (i & 15)] of word i >> 4, letter = bits 2:1 of its ASCII code (A 0, C 1, T 2, G 3 -- the alphabet of the
    // filter's k-mer codes, sketch_filter.hip pack16le -- for ANY byte, so that both formats give the filter the same codes);
    // npos: the ascending positions of the bases that are not one of ACGTacgt (they poison every k-mer that holds them, exactly
    // as in the ASCII form).  The kernels of the filtered sequence and sketch_wave_kernel read this form; every other consumer of
    // bases gets an ASCII copy made on the device (launch_unpack).
    int packed;
    const uint64_t* npos;
    uint64_t n_npos;
    const uint16_t* nbits; // packed batches in sketch_wave_kernel: bit j of word i = base 16 i + j is in npos (null when n_npos == 0):
                           // launch_mark_npos sets them before the kernel (the list itself would cost a search per tile)
    // index
    const void* slot_key; // u32[2^bits] (k <= 15) or u64[2^bits]
    const uint2* slot_rec; // {record offset, record count}; count 0 = empty slot
    const uint4* slot_first; // {record offset, record count, rec_knode of the first record, its prg | min path length of that prg << 12}:
                             // everything a candidate record needs of a slot in one load instead of three dependent ones
    uint32_t table_bits;
    const uint32_t* rec_knode; // (global k-mer node << 1) | strand
    const uint16_t* rec_prg;
    uint32_t* tile_first_read; // scratch, one entry per tile (filled by launch_sketch_probe)
    // outputs
    uint64_t* hit_key;
    uint32_t* hit_val;
    uint64_t hit_capacity;
    unsigned long long* n_hits;
    unsigned long long* n_minimizers;
    const uint32_t* pbloom; // direct kernel: Bloom tier in front of a table that does not fit L2 (nullptr: none)
    uint32_t pbloom_wbits;
    uint32_t* overflow; // bit 0: hit buffer too small, bit 1: read longer than 2^HIT_POS_BITS, bit 2: candidate slice
                        // too small, bit 3: dynamic LDS does not start at address 0 (sketch_filter_kernel), bit 4: a chunk of its schedule holds too
                        // few whole tiles, bit 5: the batch's offsets do not span [0, n_bases) (its chunk schedule was made for all of its tiles)
    // candidate form of the direct kernel (tile_cap != 0): instead of hits, every tile leaves the records
    // read_cluster_kernel wants (same layout as FilterWork::cand_info / cand_pos1 / cand_rec), in position order, in its own
    // slice of tile_cap entries; tile_count[t] = minimizers found, tile_hits[t] = their hits, tile_nmin[t] = all minimizers of the tile
    uint32_t tile_cap;
    uint64_t* tile_info;
    uint32_t* tile_pos1;
    uint4* tile_rec;
    uint32_t *tile_count, *tile_hits, *tile_nmin;
    const uint32_t* prg_min_path_len; // for the size threshold stored in the records
    const uint32_t* prg_thr;          // per PRG: floor(shortest k-mer path * fraction) (sketch_wave_kernel)
    double fraction;
    uint32_t min_cluster_size;
};

struct ClusterRec {
    uint32_t read, prg_rev, first_pos, last_pos, n, state;
};

struct ClusterArgs {
    const uint64_t* key; // sorted hits
    const uint32_t* val;
    const uint32_t* scan;   // inclusive scan of cluster-head flags
    const uint32_t* cstart; // n_clusters + 1
    const uint32_t* d_n_clusters; // device scalar
    const uint64_t* offsets;
    const uint32_t* prg_min_path_len;
    ClusterRec* clusters;
    uint32_t* order;
    int w;
    double fraction;
    uint32_t min_cluster_size;
    uint32_t* covg;
    uint32_t* prg_reads;
    unsigned long long* n_clusters_kept;
    unsigned long long* n_hits_kept;
};

// optional HIP events recorded on the launch stream immediately around the dominant kernel of a launch sequence
struct KernelTimer {
    hipEvent_t begin = nullptr, end = nullptr;
};

uint32_t sketch_tile_eval(int halo);
uint32_t sketch_n_tiles(uint64_t n_bases, int halo);
hipError_t launch_sketch_probe(const SketchArgs& a, bool wide_hash, hipStream_t stream, KernelTimer timer = {});
bool probe_compile_time_window(int k, int w); // 32-bit keys: sketch_probe_kernel<uint32_t, k, w> serves these, the sequential scan the rest
// first read that starts at or after the first staged base (tile * t_eval - halo) of every tile
hipError_t launch_tile_first_read(const uint64_t* offsets, uint32_t n_reads, int t_eval, int halo, uint32_t n_tiles, uint32_t* out,
    hipStream_t stream);
// register-resident form of the direct kernel's candidate form (sketch_wave.hip): k = 15, w in {11, 14}; one tile per wave
bool wave_kernel_applies(int k, int w);
uint32_t wave_tile_eval();
uint32_t wave_n_tiles(uint64_t n_bases);
uint32_t wave_n_slices(uint64_t n_bases); // one slice of tile_cap records per workgroup of four tiles
hipError_t launch_sketch_wave(const SketchArgs& a, hipStream_t stream, KernelTimer timer = {});
// tiles of the candidate form of the direct sequence for these parameters (whichever kernel serves them; force_lds: Switches::direct_lds)
uint32_t direct_candidate_tiles(uint64_t n_bases, int halo, int k, int w, bool wide_hash, bool force_lds); // = slices
bool direct_uses_wave_form(int k, int w, bool wide_hash, bool force_lds); // sketch_wave_kernel serves these parameters
uint32_t direct_first_read_tiles(uint64_t n_bases, int halo, int k, int w, bool wide_hash, bool force_lds); // entries of tile_first_read
// filtered form (k <= 15, w <= 16): bloom = 2^bloom_wbits words of index k-mer codes
uint32_t filter_n_tiles(uint64_t n_bases, int positions_per_lane = 32);
uint32_t filter_grid(bool level0, int n_cus, uint32_t n_tiles, uint32_t cap); // cap: Switches::ft_grid (0: none)
// device copies of FlatIndex::bloom / bloom0 (bloom0 == nullptr: no level 0)
struct BloomTables {
    const uint32_t* bloom;
    uint32_t bloom_wbits;
    const uint32_t* bloom0;
    uint32_t bloom0_wbits;
    const uint32_t* bloomr; // FlatIndex::bloomr (2^BLOOMR_WBITS words): the second stage of the retired two-kernel level-0 form; no kernel reads it
    const uint32_t* bloom0f; // level 0 and the second-stage bits in one array (the form with the second stage inside the streaming kernel)
    // middle tier (FlatIndex::mid0 / mid_bitmap / midc; nullptr: absent)
    const uint32_t* mid0 = nullptr;
    const uint32_t* mid_bitmap = nullptr;
    const uint32_t* midc = nullptr;
    uint32_t midc_wbits = 0, mid0_bits = 0;
    // small tier, second stage in the L2 (round 6; FlatIndex::blkc): split-block filter of the codes, block chosen by the group's plain 12-mer
    const uint32_t* blkc = nullptr;
    uint32_t blkc_wbits = 0;
};
// Scratch of the filtered launch sequence.  raw_pos: raw_capacity candidate positions (one slice per filter wave);
// cand_info / cand_pos1: raw_capacity entries each; small: filter_small_words() u32; max_len: device scalar that
// receives the length of the longest read holding a minimizer hit.  Overflow bit 2 (value 4) in a.overflow: a slice
// was too small.  The hits are written ordered by (read, position); a.n_hits receives their number.
struct FilterBuffers {
    uint64_t* raw_pos;
    uint64_t* cand_info;
    uint32_t* cand_pos1;
    uint4* cand_rec; // raw_capacity entries
    uint64_t raw_capacity;
    uint32_t* small;
    unsigned long long* max_len;
    // sketch_filter_kernel's tile shares (FilterWork::wave_share) for this launch, or nullptr: its built-in ones; and five zeroed device words that
    // receive ~(earliest start) and the latest end of each of the four wave classes on the 100 MHz wall clock (reported by bench.py; with the
    // static schedule the host sets the next batch's shares by them: mapper.cpp tune_filter_shares)
    const uint32_t* wave_share = nullptr;
    unsigned long long* class_clock = nullptr;
};
// How sketch_filter_kernel hands its wave tiles out (round 6).  Every workgroup owns a contiguous range of the window's tiles (an even split).
// Round 0 is static: wave i of the workgroup owns chunk i, the tiles of 16 * tpw0 split by FilterWork::wave_share (in wave order).  Rounds
// 1 .. n_rounds - 1 are dynamic: ticket k >= first_ticket[r] (drawn from a counter in the workgroup's LDS when the wave's prefetch reaches the
// end of its chunk) is the chunk of size[r] tiles that starts at tile first_tile[r] + (k - first_ticket[r]) * size[r] of the workgroup's range; the sizes
// fall from round to round so that the waves -- which do NOT run at one speed: a SIMD issues for its oldest wave first -- end together
// whatever their speeds are.  Chunk = slice: chunk k of workgroup b fills slice b * per_wg + k, and the chunks are numbered in position
// order, so the slices in order are the ordered candidate list.  A workgroup's last chunk runs to the end of its range.  Every chunk of a
// dynamic schedule holds at least two tiles that lie wholly inside the buffer (the kernel's prefetch runs two tiles ahead, into the next
// chunk at most); per_wg == 16: static only, one chunk per wave as until round 5.
constexpr int FT_MAX_ROUNDS = 8;
struct FilterSched {
    uint32_t tpw0;       // round 0: tiles per wave of an even split (0, which the host no longer makes: the kernel divides its window itself)
    uint32_t per_wg;     // chunks = slices per workgroup
    uint32_t n_tiles;    // the tiles the schedule was made for (a dynamic one: the kernel's window must be exactly tiles [0, n_tiles))
    uint32_t first_ticket[FT_MAX_ROUNDS], first_tile[FT_MAX_ROUNDS], size[FT_MAX_ROUNDS]; // [0] unused; first_ticket[r] = 0xFFFFFFFF for r >= n_rounds
    uint32_t n_rounds;
    uint32_t lds_word;   // the workgroup's ticket counter: this word of the kernel's dynamic LDS (set by the launcher; next ticket = 16 + its value)
};
// the schedule of one workgroup for the n_tiles wave tiles of a whole batch on n_wg workgroups;
// (knobs: DRPRG_FT_SCHED, switches.h)
FilterSched make_filter_sched(uint32_t n_tiles, uint32_t n_wg, const uint32_t share[4], const FilterSchedKnobs& knobs);
// sketch_filter_kernel's built-in tile shares of the four wave classes in the level-0 forms (what Mapper::tune_filter_shares starts from)
const uint32_t* filter_builtin_shares(bool mid, bool packed);
// device view of the workspace of one filtered launch sequence (filled by launch_sketch_filter)
struct FilterWork {
    const uint32_t* bloom;
    uint32_t bloom_wbits;
    const uint32_t* bloom0;  // level 0 (nullptr / 0: absent)
    uint32_t bloom0_wbits;
    const uint32_t* mid_bitmap; // middle tier: exact bitmap of the canonical index 12-mers (2^24 bits, global memory)
    const uint32_t* midc;       // middle tier: split-block Bloom filter of the index k-mer codes (2^midc_wbits blocks of 16 bytes, global memory)
    uint32_t midc_wbits;
    uint32_t read_begin, read_end; // the reads the launch sequence maps: the whole batch, [0, n_reads) (launch_sketch_filter).  The
                             // filter kernel streams the wave tiles (FT_WPOS positions each) that cover their bases, candidates
                             // outside [offsets[read_begin], offsets[read_end]) are dropped by verify_scan_kernel
    uint32_t n_slices;       // slices of the candidate buffers (= chunks of the filter kernel's schedule: its workgroups x sched.per_wg)
    // Where a slice lives (round 6: the chunks are not of one size, so neither are their slices): workgroup b's slices share slice_budget
    // entries from b * slice_budget; chunk k of it, tiles [first, end) of the workgroup's range [lo, ..), starts (first - lo) * slice_cpt +
    // k * slice_slack entries in and holds (end - first) * slice_cpt + slice_slack -- room in proportion to its tiles plus a floor for the
    // small ones (a 4-tile chunk that meets five reads from the panel).  The filter kernel leaves start and room next to the count.
    // The chunks of a dynamic schedule's last round (tickets from slice_extra_from on) hold slice_extra entries more each and start
    // (k - slice_extra_from) * slice_extra further in: a long read from the panel lying wholly inside one of those small chunks fits it.
    uint32_t slice_budget, slice_cpt, slice_slack;
    uint32_t slice_extra, slice_extra_from;
    uint64_t* raw_pos;       // global base position of a candidate k-mer, ascending per slice
    uint32_t* slice_count;   // [n_slices], clamped to the slice's room (more: overflow bit 2, the host runs the batch again)
    uint32_t* slice_base;    // [n_slices]: first entry of the slice in raw_pos
    uint32_t* slice_cap;     // [n_slices]: its room
    uint32_t* super_count;   // [MAX_SLICES], zero before the launch (counters_home_kernel clears it behind every sequence): the candidates of
                             // slices 8 s .. 8 s + 7 (what verify_scan_kernel scans)
    FilterSched sched;       // sketch_filter_kernel's chunk schedule
    uint32_t* cand_count;    // one word: verify_scan_kernel's workgroup 0 leaves the number of candidates here (the filtered sequence's
                             // writable alias of *cand_total; the direct sequence aims cand_total at its tile prefix instead)
    const uint32_t* cand_total; // the number of candidates (filtered sequence: cand_count)
    uint64_t* cand_info;     // [candidates]: slot << 32 | strand << 31 | read
    uint32_t* cand_pos1;     // [candidates]: read position + 1 of a minimizer, 0 = not a minimizer
    uint4* cand_rec;         // [candidates]: what read_cluster_kernel needs of a minimizer: first index record, number of
                             // records, group << 16 | size threshold, coverage index of the first record (0,0,.. = not a minimizer)
    uint32_t ex_grid;        // workgroups of recount_kernel / expand_kernel
    uint32_t verify_grid;    // workgroups of verify_scan_kernel: as many words of wg_hits / wg_nmin / wg_maxlen hold its totals
    uint32_t *wg_hits, *wg_nmin, *wg_maxlen, *wg_base; // [ex_grid]
    unsigned long long* max_len; // longest read that holds a minimizer hit (this batch)
    unsigned long long* class_clock; // FilterBuffers::class_clock (may be null)
    uint32_t wave_share[4];  // sketch_filter_kernel: tiles of the waves 4c .. 4c + 3 of a workgroup, in 1/256 of an even share (sum 1024); see its launch
};
constexpr uint32_t READ_NONE = 0x7FFFFFFFu; // "read" of a candidate that lies past the last whole k-mer of the buffer

// per-read clustering straight from the candidate list (read_cluster_kernel)
struct ReadClusterArgs {
    const uint32_t* prg_min_path_len;
    double fraction;
    uint32_t min_cluster_size;
    int max_diff;
    uint32_t n_prgs;
    uint32_t* covg;
    uint32_t* prg_reads;
    unsigned long long* n_clusters_kept;
    unsigned long long* n_hits_kept;
    unsigned long long* n_complex; // reads left to the generic pipeline (their candidates keep cand_pos1 != 0)
    uint32_t* chunk_counter;       // zeroed device scalar: work distribution of read_cluster_kernel
    // candidates still in their tile slices (direct sequence without tile_gather_kernel): slice_prefix != nullptr.  The ordered
    // list's entry d lives in slice s = the one with slice_prefix[s] <= d < slice_prefix[s + 1], at s * a.tile_cap + (d - slice_prefix[s]);
    // handled candidates are marked cand_pos1[d] = mark_epoch in the (otherwise unused) dense array
    const uint32_t* slice_prefix; // [n_slices + 1], exclusive scan of the slice counts
    uint32_t n_slices, mark_epoch;
    const uint32_t* block_first;  // [total / 64 + 1]: the slice that holds entry 64 m of the ordered list (tile_totals_kernel writes it into the
                                  // -- until a dense list is gathered -- unused fw.cand_info)
    // the batch totals of the candidate stage (hits, minimizers, longest read with a hit) summed by workgroup 0 of read_cluster_kernel
    // from verify_scan_kernel's per-workgroup words instead of by a kernel of their own (hit_scan_kernel: 6 us of launch + one round
    // trip; it still runs when the hits are counted again for the generic pipeline, which also needs its prefix sums)
    const uint32_t *wg_hits, *wg_nmin, *wg_maxlen;
    uint32_t n_wg;                 // 0: the totals are somebody else's business
    unsigned long long *tot_hits, *tot_minimizers, *tot_max_len;
    const uint32_t* overflow_word; // bit 2: a candidate slice overflowed (the host runs the batch again: minimizers must not count twice)
    uint32_t minpath_in_lds;         // set by launch_read_cluster: the dynamic LDS holds [n_prgs] u16 shortest paths behind the histogram
};
// from[0 .. n) -> to[0 .. n) (the device address of pinned host memory), then from[0 .. n) = 0; n <= 64.  zero != nullptr: zero[0 .. n_zero)
// = 0 as well (n_zero a multiple of 4, zero 16-byte aligned: the superblock counts of the filtered sequence)
hipError_t launch_counters_home(unsigned long long* from, unsigned long long* to, uint32_t n, hipStream_t stream, uint32_t* zero = nullptr, uint32_t n_zero = 0);
uint32_t* filter_super_counts(uint32_t* small); // the superblock counts inside a FilterBuffers::small block ...
uint32_t filter_super_words();                  // ... and how many words they are
size_t filter_small_words();
// the fields of fw that the consumers of a dense candidate list use (candidates.hip, read_cluster.hip)
void init_candidate_work(FilterWork& fw, const FilterBuffers& b, int n_cus);
// filter -> candidates -> verify -> per-read clustering of the reads that fit read_cluster_kernel (coverage, PRG read
// counts and the kept-cluster counters are updated); a.n_hits receives the number of hits of the whole batch,
// rc.n_complex the number of reads left over.  fw is filled for the two follow-up calls.  sw: the grid cap, schedule, tile shares, second
// stage and read_cluster_kernel switches
hipError_t launch_sketch_filter(const SketchArgs& a, const BloomTables& bt, int n_cus, const FilterBuffers& b, const ReadClusterArgs& rc, FilterWork& fw,
    const Switches& sw, hipStream_t stream, KernelTimer timer = {});
// leftover reads: a.n_hits receives the number of their hits, b.max_len their longest read ...
hipError_t launch_filter_recount(const SketchArgs& a, const FilterWork& fw, hipStream_t stream);
// ... and their hits are written to a.hit_key / a.hit_val ordered by (read, position)
hipError_t launch_filter_expand(const SketchArgs& a, const FilterWork& fw, hipStream_t stream);
// Candidate form of the direct sequence: launch_sketch_probe / launch_sketch_wave with a.tile_cap != 0, then read_cluster_kernel
// straight from the tile slices (*fw.cand_total: their total); it marks the candidates it handled with slices_mark (!= 0) in the dense
// fw.cand_pos1.  tile_prefix: n_tiles + 1 words; temp: scan_temp_bytes(n_tiles + 1) bytes.  a.n_hits receives the hits of the batch;
// overflow bit 2: a tile slice was too small, or the total exceeds dense_capacity (nothing was counted then).
hipError_t launch_direct_candidates(const SketchArgs& a, bool wide_hash, bool force_lds, uint32_t* tile_prefix, void* temp, size_t temp_bytes,
    uint64_t dense_capacity, const ReadClusterArgs& rc, int n_cus, FilterWork& fw, hipStream_t stream, KernelTimer timer, uint32_t slices_mark);
// the gathered list after such a batch, for the reads that were left over (handled candidates get position 0)
hipError_t launch_tile_gather_marked(const SketchArgs& a, const FilterWork& fw, const uint32_t* tile_prefix, uint32_t n_tiles, uint64_t dense_capacity,
    uint32_t mark, hipStream_t stream);
hipError_t exclusive_scan_u32(void* temp, size_t temp_bytes, const uint32_t* in, uint32_t* out, uint32_t n, hipStream_t stream);
// hits ordered by (read, pos) -> ordered by (read, prg, strand, pos), in place; meant for short reads.  key_tmp / val_tmp: n entries each,
// used for the reads with more hits than the kernel sorts in LDS.  scratch: u32 words (>= n) for the list of reads that need reordering;
// count: zeroed device scalar
hipError_t launch_read_sort(uint64_t* key, uint32_t* val, uint64_t* key_tmp, uint32_t* val_tmp, uint32_t n, uint32_t* scratch, uint64_t scratch_words,
    unsigned long long* count, hipStream_t stream);
size_t sort_temp_bytes(uint32_t n);
size_t scan_temp_bytes(uint32_t n);
hipError_t sort_hits(void* temp, size_t temp_bytes, const uint64_t* key_in, uint64_t* key_out, const uint32_t* val_in,
    uint32_t* val_out, uint32_t n, hipStream_t stream);
hipError_t launch_cluster_flags(const uint64_t* key, uint32_t n, int max_diff, uint32_t* head, uint32_t* scan, void* temp,
    size_t temp_bytes, hipStream_t stream);
hipError_t launch_cluster_starts(const uint32_t* head, const uint32_t* scan, uint32_t n, uint32_t* cstart, hipStream_t stream);
hipError_t launch_cluster_pipeline(const ClusterArgs& a, uint32_t n_hits, uint32_t n_prgs, hipStream_t stream);
hipError_t launch_vector_add_u32(uint32_t* dst, const uint32_t* src, uint64_t n, hipStream_t stream); // dst[i] += src[i]
// packed.hip: 2-bit packed reads -> ASCII (A C G T, 'N' at the positions in npos and in the 64 bytes behind the last base): what the
// direct sketch kernels and the anchor scan read.  out: n_bases + 64 bytes, 16-byte aligned.
hipError_t launch_unpack(const uint32_t* words, uint64_t n_bases, const uint64_t* npos, uint64_t n_npos, uint8_t* out, hipStream_t stream);
// bits[i >> 4] |= 1 << (i & 15) for every position i of npos below n_bases (bits: zeroed u16[ceil(n_bases / 16)], 4-byte aligned)
hipError_t launch_mark_npos(const uint64_t* npos, uint64_t n_npos, uint64_t n_bases, uint16_t* bits, hipStream_t stream);
// ... and ASCII -> packed on the device (harnesses: bench.py packs its synthetic batch with it).  words: ceil(n_bases / 16); npos: room
// for npos_cap positions, *n_npos (zeroed by the caller) counts all of them (more than npos_cap: overflow); positions come out
// unordered: sort them before use.
hipError_t launch_pack(const uint8_t* bases, uint64_t n_bases, uint32_t* words, uint64_t* npos, uint64_t npos_cap, unsigned long long* n_npos,
    hipStream_t stream);

// bam_pack.hip: a batch whose sequences are in BAM's 4-bit form (code i of "=ACMGRSVTWYHKDBN" per base, high nibble first) -> the packed
// form.  Read i is offsets[i + 1] - offsets[i] bases long, its field starts at byte seq_start[i] of seq (the fields need not be adjacent
// or in order) and the read is the field's reverse complement when reverse[i] != 0 (reverse == nullptr: none is).  words:
// ceil(n_bases / 16), tail bits of the last word clear, one 16-byte store per four words when words is 16-byte aligned.  A code other
// than A, C, G, T gets the letter of its upper-case character and is a non-ACGT position: words and positions are what launch_pack makes
// of the upper-case text of the same reads.  list: chunk_prefix[bam_pack_chunks(n_bases)] receives the number of those positions (below
// 2^32) and -- npos != nullptr -- the first npos_cap of them are written to npos, ASCENDING.  chunk_count / chunk_prefix:
// bam_pack_chunks(n_bases) + 1 words each; temp: scan_temp_bytes(bam_pack_chunks(n_bases) + 1) bytes; none is touched when !list ...
// except chunk_count, which the first launch always fills.
uint32_t bam_pack_chunks(uint64_t n_bases);
hipError_t launch_bam_pack(const uint8_t* seq, const uint64_t* seq_start, const uint64_t* offsets, const uint8_t* reverse, uint64_t n_reads, uint64_t n_bases,
    uint32_t* words, uint64_t* npos, uint64_t npos_cap, bool list, uint32_t* chunk_count, uint32_t* chunk_prefix, void* temp, size_t temp_bytes, hipStream_t stream);

// covg_cut.hip: the read at which a device batch crosses the depth cap.  out (page-locked host memory, device address): out[0] = the smallest
// i in [1, n_reads] with offsets[i] >= target (n_reads if none), out[1] = offsets[i], out[2] = how many of the n_npos ascending positions
// in npos lie below offsets[i].  One wave; n_reads >= 1.
hipError_t launch_covg_cut(const uint64_t* offsets, uint64_t n_reads, uint64_t target, const uint64_t* npos, uint64_t n_npos, unsigned long long* out,
    hipStream_t stream);

// subsample.hip: a resident sample cut to a target depth at random (the rule: include/drprg_hip.h "random subsample").
// Selection over the n reads of the sample (1 <= n < 2^32), numbered through its resident blocks.  len: u64[n], zero, then filled block by
// block by launch_subsample_lengths (reads of blocks that hold no base keep length 0).  launch_subsample_select leaves flag[i] = 1 for the
// kept reads, rank[i] = kept reads before i and boff[i] = kept bases before i (n + 1 entries each: entry n holds the totals).  key and idx:
// n + 1 entries, key_sorted, idx_sorted and csum: n entries, scratch; temp: subsample_scan_temp_bytes(n) bytes; cut: two device words.
struct SubsampleSelect {
    uint64_t n, target, seed;
    uint64_t *len, *key, *key_sorted, *csum, *boff;
    uint32_t *idx, *idx_sorted, *rank;
    uint8_t* flag;
    unsigned long long* cut;
    void* temp;
    size_t temp_bytes;
};
size_t subsample_scan_temp_bytes(uint64_t n);
hipError_t launch_subsample_lengths(const uint64_t* offsets, uint64_t n_reads, uint64_t first, uint64_t n, uint64_t* len, hipStream_t stream);
hipError_t launch_subsample_select(const SubsampleSelect& s, hipStream_t stream);
// out[2 b] = rank[first[b]], out[2 b + 1] = boff[first[b]] for n_bounds read numbers (<= n) in device memory
hipError_t launch_subsample_bounds(const uint64_t* first, uint32_t n_bounds, uint64_t n, const uint32_t* rank, const uint64_t* boff, unsigned long long* out,
    hipStream_t stream);
// Compaction of one resident block (reads first .. first + n_reads - 1 of the sample; n_reads >= 1) into a block of its new_reads kept
// reads and new_bases kept bases (what the scans say: launch_subsample_bounds).  bases / offsets / n_bases: the old block.
struct GatherEntry;
struct SubsampleBlock {
    const uint8_t* bases;
    const uint64_t* offsets;
    uint64_t n_reads, n_bases, first;
    const uint8_t* flag;
    const uint32_t* rank;
    const uint64_t* boff;
    uint64_t new_reads, new_bases;
};
// new_offsets[new_reads + 1], and per kept read its first base in the old block: src_start[new_reads] (packed blocks) or table[new_reads]
// for launch_gather_reads (ASCII blocks); either may be null.  *err (zeroed by the caller) is set to 1 by any kernel below that finds the
// scans, the block's offsets and these sizes at odds; nothing is written out of bounds then.
hipError_t launch_subsample_tables(const SubsampleBlock& b, uint64_t* new_offsets, uint64_t* src_start, GatherEntry* table, uint32_t* err, hipStream_t stream);
// words[ceil(new_bases / 16)] of the kept reads, tail bits of the last word clear; one 16-byte store per four words when words is 16-byte aligned
hipError_t launch_subsample_pack(const SubsampleBlock& b, const uint64_t* new_offsets, const uint64_t* src_start, uint32_t* words, uint32_t* err, hipStream_t stream);
// The old block's n_npos (>= 1) listed positions that lie in kept reads: chunk_prefix[subsample_npos_chunks(n_npos)] receives their number;
// then they are written at their new places, ascending.  chunk_count / chunk_prefix: subsample_npos_chunks(n_npos) + 1 words each; temp:
// scan_temp_bytes of as many.
uint32_t subsample_npos_chunks(uint64_t n_npos);
hipError_t launch_subsample_npos_count(const SubsampleBlock& b, const uint64_t* npos, uint64_t n_npos, uint32_t* chunk_count, uint32_t* chunk_prefix, void* temp,
    size_t temp_bytes, hipStream_t stream);
hipError_t launch_subsample_npos_emit(const SubsampleBlock& b, const uint64_t* npos, uint64_t n_npos, const uint32_t* chunk_prefix, uint64_t* out, uint64_t out_cap,
    hipStream_t stream);

// dedup.hip: exact duplicate reads (the rule: include/drprg_hip.h "duplicate reads").  DedupBatch (dedup_word.h): one packed batch.
// launch_dedup_keys ADDS every read's content key to key[read] (u64[n_reads], zeroed by the caller: a read of no bases keeps 0); *err
// (zeroed by the caller) is set to 1 by any kernel below that finds offsets at odds with n_bases or an index out of range, and nothing is
// written out of bounds then.  words: ceil(n_bases / 16); 16-byte loads when it is 16-byte aligned.
// Selection over the n reads of the sample (1 <= n < 2^32), numbered through its resident blocks.  loc: n entries, zero, then filled block
// by block by launch_dedup_loc (every block's words and bitmap must live until launch_dedup_select is done); key: n + 1 entries, the keys
// in [0, n).  launch_dedup_select leaves flag[i] = 0 for every read that is identical to a read before it, rank[i] = kept reads before i and
// boff[i] = kept bases before i (n + 1 entries each, entry n the totals), exactly as launch_subsample_select does.  idx: n + 1 entries,
// key_sorted and idx_sorted: n entries, scratch; temp: subsample_scan_temp_bytes(n) bytes.  key_bits (1..64): how many low bits of the
// key the sort sees; the result does not depend on it.
struct DedupLoc {
    const uint32_t* words;
    const uint16_t* bits;
    uint64_t start, len;
};
struct DedupSelect {
    uint64_t n;
    uint32_t key_bits;
    const DedupLoc* loc;
    uint64_t *key, *key_sorted, *boff;
    uint32_t *idx, *idx_sorted, *rank;
    uint8_t* flag;
    uint32_t* err;
    void* temp;
    size_t temp_bytes;
};
uint32_t dedup_tiles(uint64_t n_bases);
hipError_t launch_dedup_keys(const DedupBatch& b, unsigned long long* key, uint32_t* err, hipStream_t stream);
hipError_t launch_dedup_loc(const DedupBatch& b, uint64_t first, uint64_t n, DedupLoc* loc, uint32_t* err, hipStream_t stream);
hipError_t launch_dedup_select(const DedupSelect& s, hipStream_t stream);

// pair_overlap.hip: read-through adapters cut by mate overlap (the rule: include/drprg_hip.h "mate overlap").  The n reads of the sample
// (n < 2^32) are numbered as dedup numbers them, side 1 in [0, n1) and side 2 behind it; loc as launch_dedup_loc fills it (zero for a read
// that lies in no block; every block's words and bitmap must live until launch_pair_overlap is done).
// launch_pair_numbers: the source numbers of one block's reads, out[j] = base + i for the j-th read i that stays (flag / rank: the verdict
// and its exclusive scan, reads at or above `take` do not stay; flag null: every read stays and rank is not looked at).
// launch_pair_mates: src1 / src2 the ascending source numbers of the reads of either side that lie in blocks (m1, m2 of them), res1 / res2
// their resident numbers; mate (u32[n], filled with ~0u by the caller) receives, for both reads of every source number that both lists
// hold, the resident number of the other.
// launch_pair_overlap: shift[i] (i < n1; i32[n1]) = the chosen shift of read i's pair, PO_NO_SHIFT when none qualifies, PO_NOT_JUDGED when
// the pair is not judged; keep[i] (u64[n]) = the bases read i keeps; counts (PO_WORDS zeroed device words) receive the pair's counts (the
// caller sets PO_PAIRS and PO_READS).  *err (zeroed by the caller) is set by a mate number that is out of range or on the read's own side.
// merge (mate merging, pair_merge.hip; not beside clip): the counts are the clip's, every b of a pair with a chosen shift counts as
// emptied, and keep[] holds the NEW lengths: the insert for such a pair's a, 0 for its b.
constexpr uint32_t PO_MAX_LEN = 1024;
constexpr int32_t PO_NO_SHIFT = INT32_MIN, PO_NOT_JUDGED = INT32_MIN + 1;
enum {
    PO_PAIRS = 0, PO_JUDGED = 1, PO_ORPHANS = 2, PO_TOO_LONG = 3, PO_OVERLAPPING = 4, PO_READ_THROUGH = 5, PO_BASES_CUT = 6, PO_BASES_CLIPPED = 7,
    PO_READS_EMPTIED = 8, PO_READS = 9, PO_BASES_BEFORE = 10, PO_BASES_KEPT = 11, PO_WORDS = 12
};
struct PairOverlapArgs {
    const DedupLoc* loc;
    const uint32_t* mate;
    uint64_t n, n1;
    uint32_t min_overlap, error_milli, clip, merge;
    int32_t* shift;
    uint64_t* keep;
    unsigned long long* counts;
    uint32_t* err;
};
hipError_t launch_pair_numbers(const uint8_t* flag, const uint32_t* rank, uint64_t n_reads, uint64_t take, uint32_t base, uint64_t out_cap, uint32_t* out, uint32_t* err,
    hipStream_t stream);
hipError_t launch_pair_mates(const uint32_t* src1, const uint32_t* res1, uint32_t m1, const uint32_t* src2, const uint32_t* res2, uint32_t m2, uint64_t n, uint32_t* mate,
    uint32_t* err, hipStream_t stream);
hipError_t launch_pair_overlap(const PairOverlapArgs& a, hipStream_t stream);
// noff = the exclusive scan of keep over n_reads + 1 entries (entry n_reads of keep is read, not used): a block's new offsets.  temp:
// read_trim_temp_bytes(n_reads) bytes.
hipError_t launch_pair_offsets(const uint64_t* keep, uint64_t n_reads, uint64_t* noff, void* temp, size_t temp_bytes, hipStream_t stream);

// pair_merge.hip: overlapping mates merged into one read (the rule: include/drprg_hip.h "mate merging").  Behind launch_pair_overlap with
// merge set, on the same loc, mate, n, n1 and its shift[].  One launch places the side-1 reads [first, first + n_reads) at the base offsets
// noff[0 .. n_reads] of one destination of new_bases bases (noff from launch_pair_offsets over keep + first): every pair with a chosen shift as
// its merged read M; with `all` set every other read too, as the first noff[j + 1] - noff[j] bases it holds.  The destination is packed
// (words: ZEROED u32[ceil(new_bases / 16)] and what the caller wants behind them; nbits: the bitmap of M's unknown bases as
// launch_mark_npos lays it out, ZEROED u16[ceil(new_bases / 16) + 8], 8-byte aligned) or text (upper-case ACGT and N; `all` must be 0:
// the bytes of the other reads are the caller's to copy).  An unknown base of M carries letter 3 in the words, as an N does.  counts:
// PM_WORDS device words (zeroed by the caller once; launches add, PM_LONGEST is a maximum).  *err is set when shift, mate, loc and noff do
// not fit each other; such a read writes nothing, and nothing is written out of bounds.
enum { PM_MERGED = 0, PM_BOTH = 1, PM_AGREE = 2, PM_DISAGREE = 3, PM_FILLED = 4, PM_UNKNOWN_BOTH = 5, PM_BASES = 6, PM_LONGEST = 7, PM_WORDS = 8 };
struct PairMergeArgs {
    const DedupLoc* loc;
    const uint32_t* mate;
    const int32_t* shift;
    uint64_t n, n1, first, n_reads;
    const uint64_t* noff;
    uint64_t new_bases;
    uint32_t* words;
    uint16_t* nbits;
    uint8_t* text;
    uint32_t all;
    unsigned long long* counts;
    uint32_t* err;
};
hipError_t launch_pair_merge(const PairMergeArgs& a, hipStream_t stream);
// len[i] = keep[i] for a side-1 read i with a chosen shift, else 0 (n1 entries and one zero behind them: what launch_pair_offsets scans
// for a batch in which an unmerged pair is a read of no bases)
hipError_t launch_pair_merge_lengths(const int32_t* shift, const uint64_t* keep, uint64_t n1, uint64_t* len, hipStream_t stream);
// ASCII blocks: table[j] copies the bytes of the block's read j (first + j of the sample) to noff[j] -- keep[first + j] of them, none for
// a read with a chosen shift, whose room the merge kernel fills.  *err as launch_read_trim_fill sets it.
hipError_t launch_pair_merge_table(const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads, uint64_t n_bases, uint64_t first, uint64_t n1, const int32_t* shift,
    const uint64_t* keep, const uint64_t* noff, uint64_t new_bases, GatherEntry* table, uint32_t* err, hipStream_t stream);
// the set bits of a bitmap below n_bases: per 16 384 bases into chunk_count (base_mask_tiles(n_bases) words: what launch_base_mask_emit
// scans) and all of them ADDED to *total
hipError_t launch_pair_merge_bits_count(const uint16_t* nbits, uint64_t n_bases, uint32_t* chunk_count, unsigned long long* total, hipStream_t stream);

// pair_dedup.hip: duplicate pairs (the rule: include/drprg_hip.h "duplicate pairs").  The n resident reads (n < 2^32) are numbered as
// launch_pair_overlap numbers them (side 1 in [0, n1)); loc as launch_dedup_loc fills it and rkey as launch_dedup_keys does (both n
// entries; every block's words and bitmap must live until the call is done).  srcno[i]: the source pair of resident read i (~0u: the read
// lies in no block and belongs to no unit), mate[i]: the resident number of its mate (~0u: none); pairs: the source pairs (1 <= pairs < 2^32).
// launch_pair_dedup leaves ukey[s] = U, keep[s] = 0 for a duplicate unit and 1 for every other, copies[s] = the copies of a kept unit
// with bases and 0 for every other (pairs entries each); flag[i] = 0 for every read with bases of a duplicate unit, rank / boff as
// launch_dedup_select leaves them (n + 1 entries, as flag32 and klen); out: PD_WORDS device words, of which it writes PD_WITH_BASES,
// PD_BOTH, PD_DROPPED and the 32 levels behind PD_LEVELS (the caller sets the rest).  unit: 2 pairs entries, skey / skey_sorted / idx /
// idx_sorted / root: pairs entries, ubases: pairs bytes, changed: PD_ROUNDS + 1 words -- scratch; temp: subsample_scan_temp_bytes(max(n,
// pairs)) bytes.  *err (zeroed by the caller) is set by any index out of range, by mates that do not name each other, and by links that
// have not reached their class's first unit after PD_ROUNDS rounds; nothing is written out of bounds then.
constexpr int PD_ROUNDS = 32;
enum { PD_UNITS = 0, PD_WITH_BASES = 1, PD_BOTH = 2, PD_DROPPED = 3, PD_READS_BEFORE = 4, PD_BASES_BEFORE = 5, PD_READS_KEPT = 6, PD_BASES_KEPT = 7, PD_LEVELS = 8, PD_WORDS = 40 };
struct PairDedupArgs {
    uint64_t n, n1, pairs;
    uint32_t key_bits;
    const DedupLoc* loc;
    const unsigned long long* rkey;
    const uint32_t *srcno, *mate;
    uint32_t* unit;
    uint64_t *ukey, *skey, *skey_sorted;
    uint32_t *idx, *idx_sorted, *root, *copies;
    uint8_t *ubases, *keep, *flag;
    uint32_t *flag32, *rank;
    uint64_t *klen, *boff;
    unsigned long long* out;
    uint32_t *changed, *err;
    void* temp;
    size_t temp_bytes;
};
hipError_t launch_pair_dedup(const PairDedupArgs& a, hipStream_t stream);
// srcno[res[k]] = src[k] for the m reads of one list (launch_pair_mates' lists; srcno: n entries, filled with ~0u by the caller)
hipError_t launch_pair_source_numbers(const uint32_t* src, const uint32_t* res, uint32_t m, uint64_t n, uint32_t* srcno, uint32_t* err, hipStream_t stream);

// read_qual.hip: the read filter (the rule: include/drprg_hip.h "read filter").  qsum[i] = sum of E[quality] over read i's n_bases-indexed
// bytes of qual (qual: n_bases + 64 bytes readable; bias 33 or 0), then flag[i] = 1 for the reads the rule keeps, rank[i] = kept reads
// before i and boff[i] = kept bases before i (n_reads + 1 entries each, entry n_reads the totals: what launch_subsample_tables and the
// compaction kernels of subsample.hip read).  use_qual == false: qual and qsum are not touched.  flag32, klen: n_reads + 1 entries of
// scratch; work: RF_WORDS device words; out: RF_WORDS words the device can write (page-locked host memory, or device memory), indexed by RF_*;
// temp: read_filter_temp_bytes(n_reads) bytes.  1 <= n_reads <= MAX_BATCH_READS.
// decoy_valid != null: the decoy screen's verdict (decoy_screen.hip; the rule: include/drprg_hip.h "decoy screen") on the reads the length
// and quality tests kept, from the V and H launch_decoy_screen left in decoy_valid / decoy_hits (u32[n_reads]): a read it drops has flag 0
// like any other, so the scans see one verdict; RF_DECOY_* count the reads judged, their bases, the reads and bases dropped, and the sums of
// V and H over the judged reads.  Null (no decoy set): nothing of it is read or counted.  work and out: RF_WORDS words each.
// cplx_diff != null: the low-complexity verdict (the rule: include/drprg_hip.h "read complexity") on the reads the length and quality tests
// kept, from the D launch_read_diff left in cplx_diff (u32[n_reads]) and cplx_percent (1..100): a read it drops has flag 0 like any other,
// and the decoy screen's verdict then applies only to the reads it kept as well; RF_CPLX_* count the reads judged, their bases, and the
// reads and bases dropped.  Null: nothing of it is read or counted.
enum {
    RF_KEPT_READS = 0, RF_KEPT_BASES = 1, RF_SHORT = 2, RF_LONG = 3, RF_LOWQ = 4, RF_BAD_AT = 5 /* first bad quality byte + 1, or 0 */,
    RF_OFFSETS = 6 /* offsets at odds with n_bases */, RF_ERR = 7 /* work only: the error word of the compaction behind the filter */,
    RF_DECOY_READS = 8, RF_DECOY_BASES = 9, RF_DECOY_DROPPED = 10, RF_DECOY_DROPPED_BASES = 11, RF_DECOY_VALID = 12, RF_DECOY_HITS = 13,
    // the low-complexity filter (read_complexity.hip), all zero without it: reads judged, their bases, reads and bases dropped
    RF_CPLX_READS = 14, RF_CPLX_BASES = 15, RF_CPLX_DROPPED = 16, RF_CPLX_DROPPED_BASES = 17, RF_WORDS = 18
};
struct ReadFilterArgs {
    const uint8_t* qual;
    uint32_t bias;
    const uint64_t* offsets;
    uint64_t n_reads, n_bases;
    uint64_t min_len, max_len, T;
    bool use_qual;
    const uint32_t *decoy_valid, *decoy_hits;
    uint32_t decoy_frac_milli, decoy_min_kmers;
    const uint32_t* cplx_diff;
    uint32_t cplx_percent;
    unsigned long long* qsum;
    uint8_t* flag;
    uint32_t *flag32, *rank;
    uint64_t *klen, *boff;
    unsigned long long *work, *out;
    void* temp;
    size_t temp_bytes;
};
size_t read_filter_temp_bytes(uint64_t n_reads);
uint32_t read_qual_tiles(uint64_t n_bases);
// timer: around read_qual_kernel alone
hipError_t launch_read_filter(const ReadFilterArgs& a, hipStream_t stream, KernelTimer timer = {});

// read_trim.hip: read trimming (the rule: include/drprg_hip.h "read trimming").  begin[i], end[i]: the kept range of read i in read
// orientation ([0, 0) when empty), klen[i] its length, noff the exclusive scan of klen (n_reads + 1 entries each, entry n_reads of noff
// the kept bases).  qual (n_bases + 64 bytes readable when 16-byte aligned; bias 33 or 0), first and last (u32[n_reads], scratch) are
// touched only when qual_milli != 0; window is 1..32 then.  rev: u8[n_reads], non-zero where the quality bytes are stored mirrored, or
// null.  work: RT_WORDS device words; out: RT_WORDS words the device can write, indexed by RT_*; temp: read_trim_temp_bytes(n_reads) bytes.
// 1 <= n_reads <= MAX_BATCH_READS.  ad.n != 0: adapter trimming behind it on the same ranges (adapter_trim.hip; pts: the bases, its
// offsets, ranges and sizes are taken from here).
enum {
    RT_KEPT_BASES = 0, RT_LOST_READS = 1, RT_CUT_FRONT = 2, RT_CUT_TAIL = 3, RT_QCUT_FRONT = 4, RT_QCUT_TAIL = 5, RT_EMPTIED = 6,
    RT_BAD_AT = 7 /* first bad quality byte + 1, 0, or ~0: offsets at odds with n_bases */, RT_KEPT_NPOS = 8 /* out only */, RT_OFFSETS = 9 /* work only */,
    // adapter trimming (adapter_trim.hip), all zero without adapters: bases in the ranges the crops and the quality trim left, reads and
    // bases cut, reads emptied
    RT_AD_BASES_SEEN = 10, RT_AD_READS_CUT = 11, RT_AD_BASES_CUT = 12, RT_AD_EMPTIED = 13,
    // the same four for 5' adapters (adapter_edit.hip): the bases seen are those behind the 3' cut
    RT_FA_BASES_SEEN = 14, RT_FA_READS_CUT = 15, RT_FA_BASES_CUT = 16, RT_FA_EMPTIED = 17,
    // the same four for poly tails (poly_tail.hip): the bases seen are those behind both adapter cuts
    RT_PT_BASES_SEEN = 18, RT_PT_READS_CUT = 19, RT_PT_BASES_CUT = 20, RT_PT_EMPTIED = 21, RT_WORDS = 22 /* words of work and of out */
};
// adapter_trim.hip: what adapter_points_kernel searches.  The bases as text (n_bases + 64 bytes readable when 16-byte aligned; any other
// address is read byte by byte and never behind n_bases) or, when words != null, as a packed batch's words (ceil(n_bases / 16)) with
// nbits, the bitmap launch_mark_npos makes of its position list (null: none).  begin / end: every read's range, read orientation, counted
// from its first base; cut: u32[n_reads], the smallest matching start counted from begin, or AD_NONE.
struct AdapterPoints {
    const uint8_t* text;
    const uint32_t* words;
    const uint16_t* nbits;
    const uint64_t* offsets;
    const uint64_t *begin, *end;
    uint64_t n_reads, n_bases;
    uint32_t* cut;
};
uint32_t adapter_trim_tiles(uint64_t n_bases);
// cut := AD_NONE, adapter_points_kernel, adapter_apply_kernel: end[i] = begin[i] + cut[i] where there is a match, klen[i] (klen may be null)
// the new length, the counts ADDED to work[RT_AD_*]; work[RT_OFFSETS] is set when a range does not lie inside its read.  end is a.end.
// timer: around adapter_points_kernel alone
hipError_t launch_adapter_trim(const AdapterPoints& a, const AdapterSet& ad, uint64_t* end, uint64_t* klen, unsigned long long* work, hipStream_t stream,
    KernelTimer timer = {});
// adapter_edit.hip: the indel rule.  3' side (ad3.n != 0): cut := AD_NONE, adapter_edit_points_kernel<-1>, apply: end[i] = begin[i] + cut[i],
// counts ADDED to work[RT_AD_*]; then the 5' side (ad5.n != 0, ad5 / eq5: the adapters letter-reversed, ae_reversed) on what is left:
// cut := 0, adapter_edit_points_kernel<1>, apply: begin[i] += cut[i], counts ADDED to work[RT_FA_*].  begin and end are a.begin and a.end;
// klen[i] (klen may be null) the new length; work[RT_OFFSETS] as launch_adapter_trim.  timer3 / timer5: around either points kernel alone
uint32_t adapter_edit_tiles(uint64_t n_bases);
hipError_t launch_adapter_edit(const AdapterPoints& a, const AdapterSet& ad3, const AdapterEq& eq3, const AdapterSet& ad5, const AdapterEq& eq5, uint64_t* begin,
    uint64_t* end, uint64_t* klen, unsigned long long* work, hipStream_t stream, KernelTimer timer3 = {}, KernelTimer timer5 = {});
// poly_tail.hip: poly-tail trimming (the rule: include/drprg_hip.h "poly tails") on the same inputs (a.cut is not looked at): end[i] -= the
// longest qualifying suffix of read i's range over the letters of the set (letters: bit 0 A, 1 C, 2 G, 3 T; min_len: 2..255), klen[i] (klen
// may be null) the new length, the counts ADDED to work[RT_PT_*]; work[RT_OFFSETS] as launch_adapter_trim.  One launch; a read costs its
// tail's length plus a few bases, not its own.  end is a.end.  timer: around poly_tail_kernel
hipError_t launch_poly_tail(const AdapterPoints& a, uint32_t letters, uint32_t min_len, uint64_t* end, uint64_t* klen, unsigned long long* work, hipStream_t stream,
    KernelTimer timer = {});
struct ReadTrimArgs {
    const uint8_t* qual;
    uint32_t bias;
    const uint64_t* offsets;
    const uint8_t* rev;
    uint64_t n_reads, n_bases;
    uint64_t front, tail;
    uint32_t qual_milli, window;
    uint32_t *first, *last;
    uint64_t *begin, *end, *klen, *noff;
    unsigned long long *work, *out;
    void* temp;
    size_t temp_bytes;
    AdapterSet ad;
    AdapterPoints pts;
    uint32_t poly_letters, poly_min_len; // poly tails behind the adapters (poly_tail.hip) on pts; poly_letters == 0: none
};
// the indel rule (adapter_edit.hip) in place of the plain one: launch_read_trim's last argument, kept out of ReadTrimArgs, which goes to
// kernels by value.  ad3 and ad5 (letter-reversed; either may be empty) with their match masks; ReadTrimArgs::ad is not looked at then
struct AdapterEditSets {
    AdapterSet ad3, ad5;
    AdapterEq eq3, eq5;
};
// the block's listed non-ACGT positions (n_npos == 0: none, nothing else is looked at).  chunk_count / chunk_prefix:
// read_trim_npos_chunks(n_npos) + 1 words each; temp: scan_temp_bytes of as many.  launch_read_trim leaves the number of positions inside
// kept ranges in out[RT_KEPT_NPOS] and the scan in chunk_prefix, which launch_read_trim_npos_emit reads.
struct ReadTrimNpos {
    const uint64_t* npos;
    uint64_t n_npos;
    uint32_t *chunk_count, *chunk_prefix;
    void* temp;
    size_t temp_bytes;
};
// what the compaction kernels take: src_start[n_reads] for launch_subsample_pack, btable[n_reads] (from `bases`) and qtable[n_reads] (from
// `qual`, stored order) for launch_gather_reads; each may be null.  *err (zeroed by the caller) is set when the ranges, the scan and the
// offsets do not fit each other; such an entry copies nothing.
struct ReadTrimFill {
    const uint64_t* offsets;
    const uint8_t* rev;
    const uint64_t *begin, *end, *noff;
    uint64_t n_reads, n_bases, new_bases;
    const uint8_t *bases, *qual;
    uint64_t* src_start;
    GatherEntry *btable, *qtable;
    uint32_t* err;
};
size_t read_trim_temp_bytes(uint64_t n_reads);
uint32_t read_trim_tiles(uint64_t n_bases);
uint32_t read_trim_npos_chunks(uint64_t n_npos);
// timer: around trim_points_kernel alone
hipError_t launch_read_trim(const ReadTrimArgs& a, const ReadTrimNpos& np, hipStream_t stream, KernelTimer timer = {}, const AdapterEditSets* edit = nullptr);
hipError_t launch_read_trim_fill(const ReadTrimFill& f, hipStream_t stream);
// the count alone, for ranges the caller made itself (mate overlap): how many of np's positions lie inside the ranges of f (offsets, begin,
// end, noff, n_reads, n_bases; nothing else of f is looked at), left in np.chunk_prefix[read_trim_npos_chunks(n_npos)] with the scan
// launch_read_trim_npos_emit reads.  n_npos >= 1.
hipError_t launch_read_trim_npos_count(const ReadTrimFill& f, const ReadTrimNpos& np, hipStream_t stream);
hipError_t launch_read_trim_npos_emit(const ReadTrimFill& f, const ReadTrimNpos& np, uint64_t* out, uint64_t out_cap, hipStream_t stream);

// decoy_screen.hip: the decoy screen (the rule: include/drprg_hip.h "decoy screen").
// The table.  text: the decoy records as upper- or lower-case text, one 'N' between two records, n_text bytes and 64 readable bytes behind
// them, 16-byte aligned.  table: n_slots slots (a power of two >= 2 x the windows of the records, at least DC_MIN_SLOTS), filled with
// DC_EMPTY here; every canonical k-mer of every all-ACGT window is inserted by a 64-bit compare-and-swap, and *distinct (zeroed here)
// counts the insertions that took an empty slot.
hipError_t launch_decoy_build(const uint8_t* text, uint64_t n_text, uint32_t k, unsigned long long* table, uint64_t n_slots, unsigned long long* distinct,
    hipStream_t stream);
// found[i] = 1 iff the canonical k-mer kmers[i] is in the table
hipError_t launch_decoy_lookup(const DecoySet& d, const unsigned long long* kmers, uint64_t n, uint8_t* found, hipStream_t stream);
// The screen.  The bases in either of adapter_points_kernel's two forms: text (n_bases + 64 bytes readable when 16-byte aligned; any other
// address is read byte by byte and never behind n_bases) or, when words != null, a packed batch's words with nbits, the bitmap
// launch_mark_npos makes of its position list (null: none).  valid[r] += V, hits[r] += H of read r (u32[n_reads], zeroed by the caller).
// 1 <= n_reads <= MAX_BATCH_READS; nothing is indexed out of bounds whatever `offsets` holds.
struct DecoyScreenArgs {
    const uint8_t* text;
    const uint32_t* words;
    const uint16_t* nbits;
    const uint64_t* offsets;
    uint64_t n_reads, n_bases;
    uint32_t *valid, *hits;
};
uint32_t decoy_screen_tiles(uint64_t n_bases);
// timer: around decoy_screen_kernel
hipError_t launch_decoy_screen(const DecoyScreenArgs& a, const DecoySet& d, hipStream_t stream, KernelTimer timer = {});
// The verdict alone, for a batch no filter has seen: flag[r] = 0 for a read the rule drops, else 1; work (four zeroed device words) receives
// reads dropped, bases dropped, the sum of V and the sum of H; *err (zeroed by the caller) is set when the offsets do not ascend from 0 to n_bases.
hipError_t launch_decoy_verdict(const DecoyScreenArgs& a, const DecoySet& d, uint8_t* flag, unsigned long long* work, uint32_t* err, hipStream_t stream);

// read_complexity.hip: the low-complexity filter (the rule: include/drprg_hip.h "read complexity").  The bases in either of
// adapter_points_kernel's two forms, as the decoy screen takes them.  diff[r] = D of read r, the neighbouring pairs inside it that differ
// (u32[n_reads]; zeroed here).  1 <= n_reads <= MAX_BATCH_READS; a read is shorter than 2^32 bases (the callers refuse a block that is
// not); nothing is indexed out of bounds whatever `offsets` holds.
struct ComplexityArgs {
    const uint8_t* text;
    const uint32_t* words;
    const uint16_t* nbits;
    const uint64_t* offsets;
    uint64_t n_reads, n_bases;
    uint32_t* diff;
};
uint32_t read_complexity_tiles(uint64_t n_bases);
// timer: around read_diff_kernel
hipError_t launch_read_diff(const ComplexityArgs& a, hipStream_t stream, KernelTimer timer = {});
// The verdict alone, for a batch no filter has seen: flag[r] = 0 for a read the rule drops under percent (1..100), else 1; work (two zeroed
// device words) receives reads dropped and bases dropped; *err (zeroed by the caller) is set when the offsets do not ascend from 0 to n_bases.
hipError_t launch_complexity_verdict(const ComplexityArgs& a, uint32_t percent, uint8_t* flag, unsigned long long* work, uint32_t* err, hipStream_t stream);

// base_mask.hip: base masking (the rule: include/drprg_hip.h "base masking").  Every base whose quality byte minus bias is below min_qual
// (1..93) becomes an unknown base, in place.  qual: n_bases bytes, indexed in bases (n_bases + 64 bytes readable when 16-byte aligned; any
// other address is read byte by byte and never behind n_bases); rev: u8[n_reads], non-zero where the quality bytes are stored mirrored, or
// null.  The bases as text (the byte becomes 'N'; nothing behind n_bases is written) or, when words != null, as a packed batch's words
// (the letter becomes 3) with nbits, the bitmap launch_mark_npos made of its position list (zeroed u16[ceil(n_bases / 16) + 8], 8-byte
// aligned; never null then), into which the masked positions are ORed, and chunk_count (base_mask_tiles(n_bases) + 1 words): the set bits
// of every workgroup's 16 384 bases.  read_flag: u32[n_reads], scratch.  work: BM_WORDS device words, indexed by BM_*.
// 1 <= n_reads <= MAX_BATCH_READS; nothing is indexed out of bounds whatever `offsets` holds.
enum {
    BM_READS_MASKED = 0, BM_BASES_MASKED = 1 /* below min_qual and one of ACGTacgt */, BM_ALREADY = 2 /* below min_qual and not */,
    BM_LISTED = 3 /* packed: the length of the position list behind the mask */, BM_BAD_AT = 4 /* first bad quality byte + 1, or ~0: none */,
    BM_OFFSETS = 5 /* offsets that do not run from 0 to n_bases, or -- where a read was looked up -- do not ascend */, BM_WORDS = 8
};
struct BaseMaskArgs {
    const uint8_t* qual;
    uint32_t bias, min_qual;
    const uint64_t* offsets;
    const uint8_t* rev;
    uint64_t n_reads, n_bases;
    uint8_t* text;
    uint32_t* words;
    uint16_t* nbits;
    uint32_t *read_flag, *chunk_count;
    unsigned long long* work;
};
constexpr uint32_t BASE_MASK_TILE = 16384; // the bases under one entry of chunk_count: one workgroup of launch_base_mask and of its emit
uint32_t base_mask_tiles(uint64_t n_bases);
// timer: around base_mask_kernel
hipError_t launch_base_mask(const BaseMaskArgs& a, hipStream_t stream, KernelTimer timer = {});
// The positions of the bitmap's set bits, ascending, into out (the first out_cap of them): the scan of the chunk_count launch_base_mask
// left, then the emit.  chunk_count / chunk_prefix: base_mask_tiles(n_bases) + 1 words each; temp: scan_temp_bytes of as many.
hipError_t launch_base_mask_emit(const uint16_t* nbits, uint64_t n_bases, uint32_t* chunk_count, uint32_t* chunk_prefix, void* temp, size_t temp_bytes, uint64_t* out,
    uint64_t out_cap, hipStream_t stream);

// read_stats.hip: read statistics (the rule: include/drprg_hip.h "read statistics"; the layout: read_stats_words.h).  The reads of a batch
// counted into acc, a snapshot's RS_DEV_WORDS device accumulators (launch_read_stats_clear puts them to their start; every launch adds).
// The bases in either of adapter_points_kernel's two forms, as the decoy screen takes them (text 16-byte aligned has 64 readable bytes
// behind n_bases; any other address is read byte by byte).  qual: as base_mask.hip takes it, with rev, or null: the three quality
// sections are left alone.  flags: u8[n_reads], 0 for a read that does not count, or null; take: only reads below it count.  gcv, esum:
// u64[n_reads] scratch (esum only with qual), zeroed here.  n_reads <= MAX_BATCH_READS, n_bases < RS_MAX_BASES; nothing is indexed out of
// bounds whatever `offsets` holds: offsets that do not ascend from 0 to n_bases set acc[RS_DEV_OFFSETS].
constexpr uint64_t RS_MAX_BASES = 1ull << 32;
struct ReadStatsArgs {
    const uint8_t* text;
    const uint32_t* words;
    const uint16_t* nbits;
    const uint8_t* qual;
    uint32_t bias;
    const uint64_t* offsets;
    const uint8_t *rev, *flags;
    uint64_t n_reads, n_bases, take;
    unsigned long long *gcv, *esum, *acc;
};
uint32_t read_stats_tiles(uint64_t n_bases);
hipError_t launch_read_stats_clear(unsigned long long* acc, hipStream_t stream);
// timer: around read_stats_pos_kernel
hipError_t launch_read_stats(const ReadStatsArgs& a, hipStream_t stream, KernelTimer timer = {});

// anchor_scan.hip: reads of a resident batch that hold one of the (sorted) anchor k-mers of length A -- every such read once,
// in any order, appended to `list` (count keeps counting past list_cap).  prefilter: 2^16 bits, bit (kmer & 0xFFFF) set for every
// anchor; flags: n_reads words, zero before the launch.
struct SelectedRead {
    uint64_t offset;       // of its first base in the batch's base array
    uint32_t len, read, batch, pad;
};
hipError_t launch_anchor_scan(const uint8_t* bases, const uint64_t* offsets, uint32_t n_reads, uint64_t n_bases, const uint64_t* anchors,
    uint32_t n_anchors, uint32_t A, const uint32_t* prefilter, uint32_t batch, uint32_t* flags, unsigned long long* count, SelectedRead* list,
    uint64_t list_cap, int n_cus, hipStream_t stream);
struct GatherEntry {
    const uint8_t* src;
    uint64_t dst;
    uint32_t len, pad;
};
hipError_t launch_gather_reads(const GatherEntry* table, uint32_t n, uint8_t* out, hipStream_t stream); // out[dst .. dst+len) = src[0 .. len)

} // namespace dev
} // namespace drprg
