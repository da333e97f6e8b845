"""Writes BAM files with nothing but struct + zlib (no BAM library is assumed): header, records with chosen flags, names, CIGAR ops
and tags, BGZF members cut at chosen payload sizes, the EOF block.  A helper of the BAM tests, not a test."""
import struct
import zlib

CODES = "=ACMGRSVTWYHKDBN"
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Rec:
    """One alignment record.  seq: the text of the SEQ field as stored (letters of CODES), i.e. BEFORE any reverse complement."""

    def __init__(self, seq, flag=4, name=b"r", n_cigar=0, tags=b"", qual=None, low_nibble_pad=0):
        self.seq, self.flag, self.name, self.n_cigar, self.tags, self.qual, self.low_nibble_pad = seq, flag, name, n_cigar, tags, qual, low_nibble_pad

    def seq_bytes(self):
        c = [CODES.index(ch) for ch in self.seq]
        if len(c) & 1:
            c.append(self.low_nibble_pad)  # (the unused low nibble behind an odd l_seq: any value)
        return bytes(c[i] << 4 | c[i + 1] for i in range(0, len(c), 2))

    def encode(self, block_size_delta=0):
        l_seq = len(self.seq)
        name = self.name + b"\0"
        cigar = b"".join(struct.pack("<I", (1 + i % 7) << 4 | (i % 2)) for i in range(self.n_cigar))
        qual = self.qual if self.qual is not None else b"\xff" * l_seq
        body = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 0, 4680, self.n_cigar, self.flag, l_seq, -1, -1, 0)
        body += name + cigar + self.seq_bytes() + qual + self.tags
        return struct.pack("<I", len(body) + block_size_delta) + body


def header(text=b"@HD\tVN:1.6\tSO:unsorted\n", refs=()):
    h = b"BAM\1" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(refs))
    for name, length in refs:
        h += struct.pack("<I", len(name) + 1) + name + b"\0" + struct.pack("<I", length)
    return h


def stream(recs, **kw):
    """the uncompressed BAM stream"""
    return header(**kw) + b"".join(r.encode() for r in recs)


def bgzf(data, payload=65280, level=1, eof=True):
    """data as BGZF members of `payload` inflated bytes each (the last one shorter), + the EOF block"""
    out = []
    for at in range(0, len(data), payload):
        chunk = data[at:at + payload]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        bsize = 12 + 6 + len(comp) + 8
        assert bsize <= 65536
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", bsize - 1) + comp + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def write(path, recs, payload=65280, level=1, eof=True, **kw):
    with open(path, "wb") as fh:
        fh.write(bgzf(stream(recs, **kw), payload, level, eof))
    return path


def counts(recs):
    """what drprg_hip_bam_info reports of a file of these records"""
    skipped = [r for r in recs if r.flag & 0x900]
    kept = [r for r in recs if not r.flag & 0x900]
    return dict(records=len(recs), skipped=len(skipped), reversed=sum(1 for r in kept if r.flag & 0x10))
