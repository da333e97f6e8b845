// adapter_args.h -- --adapter SEQ (repeatable), --adapter-error E, --adapter-min-overlap O, --adapter-indels, --front-adapter SEQ (repeatable) as `pandora map | discover` and `drprg predict`
// take them (include/drprg_hip.h "adapter trimming").  Every check that needs no device is made here, so that a usage error is one before
// a device is opened: each function returns the text of the error, which names the flag, or nothing.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace drprg {

struct AdapterArgs {
    std::vector<std::string> seqs;
    std::vector<std::string> front; // --front-adapter SEQ: 5' adapters (the indel rule only)
    bool indels = false;            // --adapter-indels
    uint32_t error_milli = 100, min_overlap = 0; // (min_overlap 0: the rule's default)
    bool error_given = false, overlap_given = false;
    bool any() const { return !seqs.empty() || !front.empty(); }
    bool plain() const { return !indels && front.empty(); } // the rule of drprg_hip_set_adapters, and that entry

    std::string add(const std::string& seq)
    {
        if (seqs.size() >= 4) return "--adapter: at most 4 adapters, " + seq + " is the fifth";
        if (seq.empty() || seq.size() > 64) return "--adapter needs a sequence of 1 to 64 letters, not " + std::to_string(seq.size());
        for (char c : seq)
            if (std::string("ACGTacgt").find(c) == std::string::npos) return "--adapter: an adapter holds the letters ACGT and no other, not " + seq;
        seqs.push_back(seq);
        return {};
    }
    std::string add_front(const std::string& seq)
    {
        if (front.size() >= 4) return "--front-adapter: at most 4 5' adapters, " + seq + " is the fifth";
        if (seq.empty() || seq.size() > 64) return "--front-adapter needs a sequence of 1 to 64 letters, not " + std::to_string(seq.size());
        for (char c : seq)
            if (std::string("ACGTacgt").find(c) == std::string::npos) return "--front-adapter: an adapter holds the letters ACGT and no other, not " + seq;
        front.push_back(seq);
        return {};
    }
    // a decimal in [0, 0.5] with at most three places, held as thousandths
    std::string set_error(const std::string& v)
    {
        const std::string bad = "--adapter-error needs a decimal error rate in [0, 0.5] with at most 3 places, not " + v;
        size_t i = 0;
        uint64_t whole = 0, frac = 0, places = 0;
        bool digit = false;
        for (; i < v.size() && v[i] >= '0' && v[i] <= '9'; ++i, digit = true)
            if ((whole = whole * 10 + (uint64_t)(v[i] - '0')) > 1000) return bad;
        if (i < v.size() && v[i] == '.')
            for (++i; i < v.size() && v[i] >= '0' && v[i] <= '9'; ++i, ++places, digit = true) {
                if (places >= 3) return bad;
                frac = frac * 10 + (uint64_t)(v[i] - '0');
            }
        if (!digit || i != v.size()) return bad;
        for (; places < 3; ++places) frac *= 10;
        const uint64_t milli = whole * 1000 + frac;
        if (milli > 500) return bad;
        error_milli = (uint32_t)milli;
        error_given = true;
        return {};
    }
    std::string set_overlap(const std::string& v)
    {
        uint64_t n = 0;
        bool digit = false;
        for (char c : v) {
            if (c < '0' || c > '9' || n > 1000) return "--adapter-min-overlap needs a number of bases, not " + v;
            n = n * 10 + (uint64_t)(c - '0');
            digit = true;
        }
        if (!digit || n < 1) return "--adapter-min-overlap needs a number of bases of at least 1, not " + v;
        min_overlap = (uint32_t)n;
        overlap_given = true;
        return {};
    }
    // once every flag has been read
    std::string check() const
    {
        if (!front.empty() && !indels) return "--front-adapter needs --adapter-indels: 5' adapters exist only under the indel rule";
        if (indels && seqs.empty() && front.empty()) return "--adapter-indels needs an adapter: --adapter SEQ or --front-adapter SEQ";
        if (seqs.empty() && front.empty()) {
            if (error_given) return "--adapter-error belongs to --adapter";
            if (overlap_given) return "--adapter-min-overlap belongs to --adapter";
            return {};
        }
        size_t shortest = 64;
        for (const std::string& s : seqs) shortest = s.size() < shortest ? s.size() : shortest;
        for (const std::string& s : front) shortest = s.size() < shortest ? s.size() : shortest;
        if (overlap_given && min_overlap > shortest)
            return "--adapter-min-overlap is 1 to the length of the shortest adapter (" + std::to_string(shortest) + "), not " + std::to_string(min_overlap);
        return {};
    }
    std::vector<const char*> front_pointers() const
    {
        std::vector<const char*> p;
        for (const std::string& s : front) p.push_back(s.c_str());
        return p;
    }
    std::vector<const char*> pointers() const
    {
        std::vector<const char*> p;
        for (const std::string& s : seqs) p.push_back(s.c_str());
        return p;
    }
    // the settings to a context: the plain rule through drprg_hip_set_adapters, as ever; anything else through drprg_hip_set_adapters2
    // (the two entries are passed in: this header needs no library)
    template <typename Ctx, typename Plain, typename Full>
    int set_on(Ctx* ctx, Plain set_adapters, Full set_adapters2) const
    {
        const std::vector<const char*> p3 = pointers(), p5 = front_pointers();
        if (plain()) return set_adapters(ctx, p3.data(), (uint32_t)p3.size(), error_milli, min_overlap);
        return set_adapters2(ctx, p3.data(), (uint32_t)p3.size(), p5.data(), (uint32_t)p5.size(), error_milli, min_overlap, indels ? 1u : 0u);
    }
    std::string tag() const // for what identifies a run
    {
        std::string t = "|A" + std::to_string(error_milli) + "/" + std::to_string(min_overlap);
        for (const std::string& s : seqs) t += "/" + s;
        if (indels) t += "/indels";
        for (const std::string& s : front) t += "/5:" + s;
        return t;
    }
};

} // namespace drprg
