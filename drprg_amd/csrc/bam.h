// bam.h -- what a BAM file means as reads (include/drprg_hip.h "BAM input"), host side: the record walker behind
// the BGZF inflate and the 4-bit code -> text conversion of the paths that want text on the host.  This build's own rule -- the
// reference refuses BAM --, restating from memory what `samtools fastq` does by default.
//
// A record: block_size u32 | refID pos i32 | l_read_name mapq u8 | bin n_cigar_op flag u16 | l_seq u32 | next_refID next_pos tlen i32 |
// read_name | cigar u32[n_cigar_op] | seq u8[(l_seq + 1) / 2] | qual u8[l_seq] | tags.  All little endian; block_size counts what follows it.
// SEQ: code i of "=ACMGRSVTWYHKDBN" per base, high nibble first.  Only flag, l_seq and seq are looked at.
#pragma once
#include "common.h"
#include <cstddef>
#include <cstdint>

namespace drprg {
namespace bam {

constexpr uint32_t FIXED_BYTES = 32;          // of a record behind block_size
constexpr uint32_t MAX_BLOCK_SIZE = 1u << 30; // a block_size beyond this is taken for garbage
constexpr uint32_t MAX_READ_BASES = 1u << 23; // dev::HIT_POS_BITS: longer reads are refused everywhere
constexpr uint16_t FLAG_REVERSE = 0x10, FLAG_SECONDARY = 0x100, FLAG_SUPPLEMENTARY = 0x800;
extern const char CODE_LETTER[17];            // "=ACMGRSVTWYHKDBN"

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline bool is_magic(const uint8_t* p, size_t n) { return n >= 4 && p[0] == 'B' && p[1] == 'A' && p[2] == 'M' && p[3] == 1; }
// the complement in code space: the four bits reversed (A=1 <-> T=8, C=2 <-> G=4, M <-> K, ...)
inline uint8_t complement(uint8_t c) { return (uint8_t)((c & 1) << 3 | (c & 2) << 1 | (c & 4) >> 1 | (c & 8) >> 3); }
inline bool is_base(uint8_t c) { return c == 1 || c == 2 || c == 4 || c == 8; }

// Bytes of the header (magic, text, reference list) at the start of the inflated stream [p, p + n), or 0: the header runs past n and
// more of the stream is needed.  Throws DRPRG_EFORMAT when p does not start with the magic or a length field is negative.
size_t header_bytes(const uint8_t* p, size_t n);

// How many bytes of [p, p + n) the whole records at its start take (p is a record start): the block_size chain is hopped, no other byte
// is touched.  A record that runs past n -- in any field, its block_size word included -- is left out.  Throws DRPRG_EFORMAT for a
// block_size below the fixed part or beyond MAX_BLOCK_SIZE.
size_t whole_records(const uint8_t* p, size_t n);

struct Record {
    const uint8_t* seq = nullptr; // (l_seq + 1) / 2 bytes
    uint32_t l_seq = 0;
    uint16_t flag = 0;
    size_t bytes = 0; // of the whole record, block_size word included
    bool skipped() const { return (flag & (FLAG_SECONDARY | FLAG_SUPPLEMENTARY)) != 0; }
    bool reverse() const { return (flag & FLAG_REVERSE) != 0; }
};
// The record at p (whole_records has said it is whole).  Throws DRPRG_EFORMAT when block_size is smaller than the fixed part + name +
// cigar + seq + qual, DRPRG_EOVERFLOW for a read of more than MAX_READ_BASES bases.
Record parse_record(const uint8_t* p);

// the read as upper-case text: out[0, l_seq) (the reverse complement when `reverse`)
void to_text(const uint8_t* seq, uint32_t l_seq, bool reverse, char* out);
// how many of its codes are not A, C, G or T (the low nibble behind an odd l_seq does not count)
uint64_t count_non_acgt(const uint8_t* seq, uint32_t l_seq);

} // namespace bam
} // namespace drprg
