// capi_reduce.cpp -- several devices: the sum of their vectors inside one context, and the RCCL communicator entries for one context per process.
#include "capi_ctx.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace drprg;

// Sum of the per-device coverage vectors of a multi-device context into its first device, on the devices (SURVEY.md section 8e:
// "one ncclReduce(sum, u32) after the last batch").  All devices distinct and RCCL present: one communicator over them
// (ncclCommInitAll, kept by the context) and two ncclReduce calls (coverage, reads per PRG) per device inside one group.  A
// device listed twice (what the one-GPU tests do), no RCCL, or DRPRG_HIP_NO_RCCL=1: peer copy into device 0 + an add kernel,
// device after device.  Then the other devices' vectors are cleared and their counters folded into the context.
void drprg::reduce_devices(drprg_hip_ctx* ctx)
{
    if (ctx->extra.empty() || !ctx->mapper) return;
    Mapper& m = *ctx->mapper;
    std::vector<Mapper*> all { &m };
    for (auto& e : ctx->extra) all.push_back(e.get());
    for (Mapper* x : all) x->sync();
    bool distinct = true;
    for (size_t i = 0; i < all.size(); ++i)
        for (size_t j = i + 1; j < all.size(); ++j) distinct &= all[i]->device() != all[j]->device();
    const char* no = std::getenv("DRPRG_HIP_NO_RCCL");
    std::string why;
    const Rccl* r = (distinct && !(no && *no && *no != '0')) ? Rccl::get(&why) : nullptr;
    bool done = false;
    auto chk = [&](int rc, const char* what) {
        if (rc != Rccl::Success) throw Error(DRPRG_EIO, std::string("RCCL ") + what + ": " + (r && r->GetErrorString ? r->GetErrorString(rc) : "error"));
    };
    if (r) {
        if (ctx->comms.empty()) {
            std::vector<int> devs;
            for (Mapper* x : all) devs.push_back(x->device());
            std::vector<Rccl::Comm> comms(all.size(), nullptr);
            const int rc = r->CommInitAll(comms.data(), (int)all.size(), devs.data());
            if (rc == Rccl::Success) ctx->comms = comms;
            else { // no communicator (nothing has been touched yet): the device add path below
                why = std::string("ncclCommInitAll: ") + (r->GetErrorString ? r->GetErrorString(rc) : "error");
                std::fprintf(stderr, "drprg-hip: warning: %s; summing the devices' vectors by peer copies\n", why.c_str());
                r = nullptr;
            }
        }
    }
    if (r) {
        // one ncclReduce per device over [coverage | reads per PRG] (one allocation: Mapper).  A group that was opened is
        // always closed: the first failure is remembered and thrown behind ncclGroupEnd, and the context is marked so that
        // nothing reads vectors of which some may be reduced and others not (drprg_hip_reset clears the mark).
        const size_t nv = 2 * (size_t)m.n_knodes() + m.n_prgs();
        chk(r->GroupStart(), "ncclGroupStart");
        int first_rc = Rccl::Success;
        const char* first_what = "";
        for (size_t d = 0; d < all.size() && first_rc == Rccl::Success; ++d) {
            if (hipSetDevice(all[d]->device()) != hipSuccess) {
                first_rc = -1;
                first_what = "hipSetDevice";
                break;
            }
            first_rc = r->Reduce(all[d]->d_covg(), all[d]->d_covg(), nv, Rccl::Uint32, Rccl::Sum, 0, ctx->comms[d], all[d]->stream());
            first_what = "ncclReduce";
        }
        const int end_rc = r->GroupEnd();
        if (first_rc != Rccl::Success || end_rc != Rccl::Success) {
            ctx->sample.needs_reset = true;
            if (first_rc == -1) throw Error(DRPRG_EIO, "hipSetDevice failed inside the reduce (drprg_hip_reset the context)");
            chk(first_rc, first_what);
            chk(end_rc, "ncclGroupEnd");
        }
        for (Mapper* x : all) {
            if (hipSetDevice(x->device()) != hipSuccess || hipStreamSynchronize(x->stream()) != hipSuccess) throw Error(DRPRG_EIO, "stream synchronisation after ncclReduce failed");
        }
        ctx->reduce_how = "rccl: ncclReduce(sum, u32) over " + std::to_string(all.size()) + " devices";
        done = true;
    }
    if (!done) {
        for (auto& e : ctx->extra) m.add_vectors_from(*e);
        ctx->reduce_how = std::string("device add: peer copy + add kernel per device (") + (distinct ? (why.empty() ? "RCCL switched off" : why) : "a device is listed twice") + ")";
    }
    for (auto& e : ctx->extra) {
        ctx->sample.extra_counts += e->counters();
        e->reset_coverage(false); // (its vectors are in the sum now; the reads it keeps in HBM stay)
    }
    ctx->sample.host_coverage_valid = false;
}

extern "C" {

int drprg_hip_reduce(drprg_hip_ctx* ctx)
{
    API_BEGIN(ctx)
    need_mapper(ctx);
    reduce_devices(ctx);
    API_END(ctx)
}

int drprg_hip_reduce_info(const drprg_hip_ctx* ctx, char* out, size_t cap)
{
    if (!ctx || !out || cap == 0) return DRPRG_EINVAL;
    std::snprintf(out, cap, "%s", ctx->reduce_how.c_str());
    return DRPRG_OK;
}

int drprg_hip_comm_unique_id(uint8_t id[128])
{
    if (!id) return DRPRG_EINVAL;
    std::string why;
    const Rccl* r = Rccl::get(&why);
    if (!r) return thread_error(DRPRG_ENODEV, why); // (no context to leave the reason in: the thread's last error)
    Rccl::UniqueId u;
    const int rc = r->GetUniqueId(&u);
    if (rc != Rccl::Success) return thread_error(DRPRG_EIO, std::string("ncclGetUniqueId: ") + r->GetErrorString(rc));
    std::memcpy(id, u.internal, sizeof u.internal);
    return DRPRG_OK;
}

int drprg_hip_comm_init_rank(void** comm, int nranks, const uint8_t id[128], int rank, int device)
{
    if (!comm || !id || nranks < 1 || rank < 0 || rank >= nranks || device < 0) return DRPRG_EINVAL;
    std::string why;
    const Rccl* r = Rccl::get(&why);
    if (!r) return thread_error(DRPRG_ENODEV, why); // (no context to leave the reason in: the thread's last error)
    if (hipSetDevice(device) != hipSuccess) return thread_error(DRPRG_ENODEV, "hipSetDevice failed");
    Rccl::UniqueId u;
    std::memcpy(u.internal, id, sizeof u.internal);
    Rccl::Comm c = nullptr;
    const int rc = r->CommInitRank(&c, nranks, u, rank);
    if (rc != Rccl::Success) return thread_error(DRPRG_EIO, std::string("ncclCommInitRank: ") + r->GetErrorString(rc));
    *comm = c;
    return DRPRG_OK;
}

int drprg_hip_comm_destroy(void* comm)
{
    if (!comm) return DRPRG_OK;
    const Rccl* r = Rccl::get();
    if (!r) return DRPRG_ENODEV;
    return r->CommDestroy(comm) == Rccl::Success ? DRPRG_OK : DRPRG_EIO;
}

int drprg_hip_allreduce(drprg_hip_ctx* ctx, void* comm, void* d_covg, void* d_prg_reads, void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!comm) throw Error(DRPRG_EINVAL, "null communicator");
    std::string why;
    const Rccl* r = Rccl::get(&why);
    if (!r) throw Error(DRPRG_ENODEV, why);
    // The context's own accumulators: a batch queued by map_device_async may still need the host (leftover reads) before its
    // vector is final, so it is completed first.  A caller's own buffers: the caller orders the reduce behind the batch that
    // filled them (the contract of drprg_hip_map_device_async says when that batch is done) -- waiting here for the batch in
    // flight would serialise the reduce of batch i with the mapping of batch i+1.  But if the batch in flight is the one that fills
    // the very buffers being reduced, the reduce completes it, as it did before round 4 (its vector may still be waiting for an
    // overflow re-run or the leftover pipeline): the caller cannot have meant to sum an unfinished vector.
    if (!d_covg || m.pending_writes_to((const uint32_t*)d_covg, (const uint32_t*)d_prg_reads)) m.sync();
    if (hipSetDevice(m.device()) != hipSuccess) throw Error(DRPRG_EIO, "hipSetDevice failed");
    uint32_t* c = d_covg ? (uint32_t*)d_covg : m.d_covg();
    uint32_t* p = d_prg_reads ? (uint32_t*)d_prg_reads : m.d_prg_reads();
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : m.stream();
    auto chk = [&](int rc, const char* what) {
        if (rc != Rccl::Success) throw Error(DRPRG_EIO, std::string("RCCL ") + what + ": " + r->GetErrorString(rc));
    };
    const size_t nc = 2 * (size_t)m.n_knodes(), np = m.n_prgs();
    if (p == c + nc) {
        // the sample's additive state is ONE vector [coverage | reads per PRG] -- the context's accumulators are laid out that
        // way, and so is a caller's buffer of drprg_hip_coverage_size's n_covg + n_prgs words -- : a single ncclAllReduce
        chk(r->AllReduce(c, c, nc + np, Rccl::Uint32, Rccl::Sum, comm, st), "ncclAllReduce");
        ctx->reduce_how = "rccl: one ncclAllReduce(sum, u32) of " + std::to_string(nc + np) + " words";
    } else {
        // two separate buffers of the caller's: one group of two (closed whatever happens inside)
        chk(r->GroupStart(), "ncclGroupStart");
        const int rc1 = r->AllReduce(c, c, nc, Rccl::Uint32, Rccl::Sum, comm, st);
        const int rc2 = rc1 == Rccl::Success ? r->AllReduce(p, p, np, Rccl::Uint32, Rccl::Sum, comm, st) : rc1;
        const int rc3 = r->GroupEnd();
        chk(rc1, "ncclAllReduce");
        chk(rc2, "ncclAllReduce");
        chk(rc3, "ncclGroupEnd");
        ctx->reduce_how = "rccl: two grouped ncclAllReduce(sum, u32) (separate buffers)";
    }
    ctx->sample.host_coverage_valid = false; // (asynchronous on the stream: the caller synchronises it, or reads through this context, which does)
    API_END(ctx)
}

} // extern "C"
