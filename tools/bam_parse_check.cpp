// bam_parse_check.cpp -- the host side of the BAM input (csrc/bam.cpp behind csrc/ingest.cpp) as a stand-alone program, for a sanitizer
// build: every file named on the command line is parsed in both forms the ingest has for BAM -- as upper-case text, and in BAM's own
// 4-bit form, which is turned into text here with the same rule -- unordered and in file order, and the two must agree.  A malformed
// file must end in an error code and a message.  No device is touched.  Build and run (tools/README.md):
//   hipcc -O1 -g -std=c++17 -Iinclude -fsanitize=address,undefined -x c++ tools/bam_parse_check.cpp drprg_amd/csrc/{ingest,bam,pack,pgunzip}.cpp \
//       -o build/bam_parse_check -lz -ldl -lpthread && build/bam_parse_check file.bam ...
#include "../drprg_amd/csrc/bam.h"
#include "../drprg_amd/csrc/ingest.h"
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

using namespace drprg;

namespace {

struct Result {
    int code = 0;
    std::string message;
    uint64_t reads = 0, bases = 0, digest = 0, non_acgt = 0;
    IngestStats st;
};

uint64_t fnv(const uint8_t* p, uint64_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (uint64_t j = 0; j < n; ++j) h = (h ^ p[j]) * 1099511628211ull;
    return h;
}

Result parse(const std::string& path, int threads, bool native, bool ordered)
{
    Result r;
    std::mutex mu;
    auto take = [&](const PinnedBatch& b) {
        std::vector<char> text;
        uint64_t digest = 0, bad = 0;
        for (uint64_t i = 0; i < b.n_reads; ++i) {
            const uint64_t len = b.offsets[i + 1] - b.offsets[i];
            const uint8_t* s = b.bases + b.offsets[i];
            if (b.bam) {
                text.resize(len);
                bam::to_text(b.bases + b.seq_start[i], (uint32_t)len, b.reverse[i] != 0, text.data());
                s = reinterpret_cast<const uint8_t*>(text.data());
            }
            for (uint64_t j = 0; j < len; ++j) bad += !(s[j] == 'A' || s[j] == 'C' || s[j] == 'G' || s[j] == 'T');
            digest += fnv(s, len);
        }
        std::lock_guard<std::mutex> g(mu);
        if (b.bam && (b.n_npos != bad || b.npos != nullptr)) r.code = -1000; // the parser thread's own count of the non-ACGT codes
        r.digest += digest;
        r.non_acgt += bad;
        r.reads += b.n_reads;
        r.bases += b.n_bases;
    };
    IngestHooks hooks;
    hooks.bam_native = native;
    hooks.concurrent_submit = true;
    hooks.submit = take;
    if (ordered)
        hooks.submit_in_order = [&](const PinnedBatch& b) {
            take(b);
            return true;
        };
    try {
        r.st = ingest_fastx(path, threads, hooks);
        if (r.st.reads != r.reads || r.st.bases != r.bases) r.code = -1001;
    } catch (const Error& e) {
        r.code = e.code;
        r.message = e.what();
    }
    return r;
}

} // namespace

int main(int argc, char** argv)
{
    int disagreements = 0, errors = 0;
    for (int a = 1; a < argc; ++a) {
        const Result first = parse(argv[a], 1, false, false);
        bool same = true;
        for (int threads : { 1, 5 })
            for (int native = 0; native < 2; ++native)
                for (int ordered = 0; ordered < 2; ++ordered) {
                    const Result r = parse(argv[a], threads, native != 0, ordered != 0);
                    same = same && r.code == first.code && (r.code != 0 || (r.reads == first.reads && r.bases == first.bases && r.digest == first.digest && r.non_acgt == first.non_acgt));
                    same = same && (r.code == 0 || !r.message.empty()) && r.code > -1000;
                }
        if (first.code) {
            ++errors;
            std::printf("%s: error %d: %s%s\n", argv[a], first.code, first.message.c_str(), same ? "" : "  DISAGREEMENT between the forms");
        } else
            std::printf("%s: %s reads=%llu bases=%llu digest=%016llx non_acgt=%llu records=%llu skipped=%llu reversed=%llu%s\n", argv[a], first.st.bam ? "BAM" : "text",
                (unsigned long long)first.reads, (unsigned long long)first.bases, (unsigned long long)first.digest, (unsigned long long)first.non_acgt,
                (unsigned long long)first.st.bam_records, (unsigned long long)first.st.bam_skipped, (unsigned long long)first.st.bam_reversed,
                same ? "" : "  DISAGREEMENT between the forms");
        disagreements += !same;
    }
    std::printf("%d files, %d ended in an error, %d disagreements\n", argc - 1, errors, disagreements);
    return disagreements ? 1 : 0;
}
