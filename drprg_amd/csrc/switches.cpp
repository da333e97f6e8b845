// switches.cpp -- the one reader of the hot path's DRPRG_* switches (switches.h).
#include "switches.h"
#include <cstdio>
#include <cstdlib>
#include <string>

namespace drprg {

Switches read_switches()
{
    Switches s;
    if (const char* e = std::getenv("DRPRG_FT_SCHED")) {
        if (std::string(e) == "static") s.ft_sched.is_static = true;
        else {
            unsigned a = 0, b = 0, c = 0, g = 64;
            const int got = std::sscanf(e, "%u,%u,%u,%u", &a, &b, &c, &g);
            if (got >= 3 && a >= 1 && a <= 250 && b >= 17 && b <= 1024 && c >= 4 && c <= 4096 && g >= 8) {
                s.ft_sched.f = a;
                s.ft_sched.d = b;
                s.ft_sched.m = c;
                s.ft_sched.min_avg = g;
            }
        }
    }
    if (const char* e = std::getenv("DRPRG_FT_GRID")) {
        const int cap = std::atoi(e);
        if (cap >= 1) s.ft_grid = (uint32_t)cap;
    }
    if (const char* e = std::getenv("DRPRG_FT_SHARE")) {
        s.ft_share_pinned = true;
        double v[4] = { 1, 1, 1, 1 };
        if (std::sscanf(e, "%lf,%lf,%lf,%lf", &v[0], &v[1], &v[2], &v[3]) == 4 && v[0] > 0 && v[1] > 0 && v[2] > 0 && v[3] > 0) {
            const double sum = v[0] + v[1] + v[2] + v[3];
            uint32_t acc = 0;
            for (int c = 0; c < 3; ++c) acc += s.ft_share[c] = (uint32_t)(1024.0 * v[c] / sum + 0.5);
            s.ft_share[3] = 1024u - acc;
        }
    }
    if (const char* e = std::getenv("DRPRG_FILTER_STAGE2"); e && *e) s.stage2 = std::string(e) == "l2" ? Stage2::l2 : Stage2::lds;
    if (const char* e = std::getenv("DRPRG_DIRECT_FORM")) s.direct_lds = std::string(e) == "lds";
    if (const char* e = std::getenv("DRPRG_FT_DEBUG")) s.skip_read_cluster = (std::atoi(e) & 8) != 0;
    if (const char* e = std::getenv("DRPRG_HIP_MIN_CAPACITY")) s.min_capacity = std::strtoull(e, nullptr, 10);
    s.force_mid_tier = std::getenv("DRPRG_FORCE_MID_TIER") != nullptr;
    if (const char* e = std::getenv("DRPRG_MID_MAX_RECORDS")) s.mid_max_records = (size_t)std::strtoull(e, nullptr, 10);
    return s;
}

} // namespace drprg
