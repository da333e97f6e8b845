// bam.cpp -- see bam.h
#include "bam.h"

namespace drprg {
namespace bam {

const char CODE_LETTER[17] = "=ACMGRSVTWYHKDBN";

size_t header_bytes(const uint8_t* p, size_t n)
{
    if (n < 4) return 0;
    if (!is_magic(p, n)) throw Error(DRPRG_EFORMAT, "BGZF stream does not start with the BAM magic");
    if (n < 8) return 0;
    const uint32_t l_text = le32(p + 4);
    if (l_text > 0x7FFFFFFFu) throw Error(DRPRG_EFORMAT, "BAM header: negative text length");
    size_t at = 8 + (size_t)l_text;
    if (at + 4 > n) return 0;
    const uint32_t n_ref = le32(p + at);
    if (n_ref > 0x7FFFFFFFu) throw Error(DRPRG_EFORMAT, "BAM header: negative reference count");
    at += 4;
    for (uint32_t i = 0; i < n_ref; ++i) {
        if (at + 4 > n) return 0;
        const uint32_t l_name = le32(p + at);
        if (l_name > 0x7FFFFFFFu) throw Error(DRPRG_EFORMAT, "BAM header: negative reference name length");
        at += 4 + (size_t)l_name + 4; // name, l_ref
        if (at > n) return 0;
    }
    return at;
}

size_t whole_records(const uint8_t* p, size_t n)
{
    size_t at = 0;
    while (n - at >= 4) {
        const uint32_t block_size = le32(p + at);
        if (block_size < FIXED_BYTES) throw Error(DRPRG_EFORMAT, "BAM record: block_size is smaller than the fixed part of a record");
        if (block_size > MAX_BLOCK_SIZE) throw Error(DRPRG_EFORMAT, "BAM record: block_size is beyond 1 GB");
        if ((size_t)block_size > n - at - 4) break;
        at += 4 + (size_t)block_size;
    }
    return at;
}

Record parse_record(const uint8_t* p)
{
    const uint32_t block_size = le32(p);
    const uint32_t l_read_name = p[12];
    const uint32_t n_cigar_op = (uint32_t)p[16] | (uint32_t)p[17] << 8;
    Record r;
    r.flag = (uint16_t)((uint32_t)p[18] | (uint32_t)p[19] << 8);
    r.l_seq = le32(p + 20);
    if (r.l_seq > 0x7FFFFFFFu) throw Error(DRPRG_EFORMAT, "BAM record: negative l_seq");
    const uint64_t need = (uint64_t)FIXED_BYTES + l_read_name + 4ull * n_cigar_op + ((uint64_t)r.l_seq + 1) / 2 + r.l_seq;
    if (need > block_size) throw Error(DRPRG_EFORMAT, "BAM record: block_size is smaller than its name, cigar, sequence and qualities");
    if (r.l_seq > MAX_READ_BASES && !r.skipped()) throw Error(DRPRG_EOVERFLOW, "a read of the BAM file is longer than 2^23 bases");
    r.seq = p + 4 + FIXED_BYTES + l_read_name + 4 * (size_t)n_cigar_op;
    r.bytes = 4 + (size_t)block_size;
    return r;
}

void to_text(const uint8_t* seq, uint32_t l_seq, bool reverse, char* out)
{
    if (!reverse) {
        for (uint32_t i = 0; i < l_seq; ++i) out[i] = CODE_LETTER[(seq[i >> 1] >> ((~i & 1) << 2)) & 15];
    } else {
        for (uint32_t i = 0; i < l_seq; ++i) {
            const uint32_t q = l_seq - 1 - i;
            out[i] = CODE_LETTER[complement((seq[q >> 1] >> ((~q & 1) << 2)) & 15)];
        }
    }
}

uint64_t count_non_acgt(const uint8_t* seq, uint32_t l_seq)
{
    // 0xFEE9 has bit c set for every code c that is not 1, 2, 4 or 8
    uint64_t n = 0;
    for (uint32_t i = 0; i < l_seq / 2; ++i) n += ((0xFEE9u >> (seq[i] >> 4)) & 1u) + ((0xFEE9u >> (seq[i] & 15)) & 1u);
    if (l_seq & 1) n += (0xFEE9u >> (seq[l_seq / 2] >> 4)) & 1u;
    return n;
}

} // namespace bam
} // namespace drprg
