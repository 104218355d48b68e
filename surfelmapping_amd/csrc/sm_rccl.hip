// sm_rccl.hip -- the built-in RCCL collective of sharded streams and rigs (sm_shard_rccl_*).  The library is bound at run
// time (dlopen), never linked.
#include "sm_ctx.h"

#include <dlfcn.h>
#include <link.h>
#include <rccl/rccl.h>      // types and enums only

#include <mutex>

using namespace sm;

namespace {

struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rccl_mu;

int find_rccl(struct dl_phdr_info *info, size_t, void *data)
{
    auto *v = static_cast<std::string *>(data);
    if (v->empty() && info->dlpi_name && std::strstr(info->dlpi_name, "librccl")) *v = info->dlpi_name;
    return 0;
}

// RCCL is bound at run time: the copy already mapped into the process if there is one (a PyTorch process has its own
// bundled librccl; two RCCLs would work but the one that is there already shares the HIP runtime for certain), else ROCm's.
int load_rccl()
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return SM_OK;
    std::string loaded;
    dl_iterate_phdr(find_rccl, &loaded);
    void *h = nullptr;
    // SM_RCCL_LIB: an explicit copy (surfelmapping_amd.capi names PyTorch's bundled one when it pre-loaded PyTorch's HIP
    // runtime: RCCL and the runtime then come from the same build)
    if (const char *e = std::getenv("SM_RCCL_LIB")) { if (e[0]) { h = dlopen(e, RTLD_NOW | RTLD_LOCAL); if (h) loaded = e; } }
    if (!h && !loaded.empty()) h = dlopen(loaded.c_str(), RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) { g_err = std::string("RCCL not found: ") + (dlerror() ? dlerror() : "dlopen failed"); return SM_E_UNSUPPORTED; }
    g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    g_rccl.AllReduce = reinterpret_cast<decltype(g_rccl.AllReduce)>(dlsym(h, "ncclAllReduce"));
    g_rccl.AllGather = reinterpret_cast<decltype(g_rccl.AllGather)>(dlsym(h, "ncclAllGather"));
    g_rccl.CommCount = reinterpret_cast<decltype(g_rccl.CommCount)>(dlsym(h, "ncclCommCount"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.AllGather || !g_rccl.CommCount || !g_rccl.CommDestroy) {
        g_err = "RCCL: missing symbols in " + (loaded.empty() ? std::string("librccl.so") : loaded);
        return SM_E_UNSUPPORTED;
    }
    g_rccl.lib = h;
    return SM_OK;
}

int rccl_collective(void *user, const void *send, void *recv, size_t count, int op, void *stream)
{
    sm_ctx *s = static_cast<sm_ctx *>(user);
    const ncclResult_t r = op == SM_COLL_GATHER
        ? g_rccl.AllGather(send, recv, count, ncclUint64, static_cast<ncclComm_t>(s->ss_comm), static_cast<hipStream_t>(stream))
        : g_rccl.AllReduce(send, recv, count, ncclUint64, op == SM_COLL_MIN ? ncclMin : ncclSum,
                           static_cast<ncclComm_t>(s->ss_comm), static_cast<hipStream_t>(stream));
    if (r != ncclSuccess) {
        g_err = std::string(op == SM_COLL_GATHER ? "ncclAllGather: " : "ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "failed");
        return SM_E_HIP;
    }
    return SM_OK;
}

}  // namespace

extern "C" {

int sm_shard_rccl_unique_id(void *out128)
{
    if (!out128) return SM_E_ARG;
    int rc = load_rccl();
    if (rc) return rc;
    ncclUniqueId id;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    const ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != ncclSuccess) { g_err = "ncclGetUniqueId failed"; return SM_E_HIP; }
    memcpy(out128, &id, 128);
    return SM_OK;
}

int sm_shard_rccl_init(sm_ctx *s, const void *id128)
{
    if (!s || !id128 || !(s->ss_on || s->rig_on)) { g_err = "sm_shard_rccl_init: call sm_shard_stream_configure or sm_rig_configure first"; return SM_E_ARG; }
    HIPCK(hipSetDevice(s->cfg.device));
    if (hip_runtime_conflict("sm_shard_rccl_init")) return SM_E_HIP;
    int rc = load_rccl();
    if (rc) return rc;
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = g_rccl.CommInitRank(&comm, s->ss_world, id, s->ss_rank);
    if (r != ncclSuccess) { g_err = std::string("ncclCommInitRank: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "failed"); return SM_E_HIP; }
    s->ss_comm = comm;
    s->ss_coll = rccl_collective; s->ss_user = s;
    return SM_OK;
}

int sm_shard_rccl_nranks(sm_ctx *s)
{
    if (!s) return SM_E_ARG;
    if (!s->ss_comm || !g_rccl.CommCount) { g_err = "sm_shard_rccl_nranks: no RCCL communicator on this context"; return SM_E_ARG; }
    int n = 0;
    const ncclResult_t r = g_rccl.CommCount(static_cast<ncclComm_t>(s->ss_comm), &n);
    if (r != ncclSuccess) { g_err = "ncclCommCount failed"; return SM_E_HIP; }
    return n;
}

int sm_shard_rccl_finalize(sm_ctx *s)
{
    if (!s) return SM_E_ARG;
    if (s->ss_comm && g_rccl.CommDestroy) {
        HIPCK(hipSetDevice(s->cfg.device));
        HIPCK(hipStreamSynchronize(s->stream));
        (void)g_rccl.CommDestroy(static_cast<ncclComm_t>(s->ss_comm));
    }
    s->ss_comm = nullptr;
    if (s->ss_coll == rccl_collective) { s->ss_coll = nullptr; s->ss_user = nullptr; }
    return SM_OK;
}

}  // extern "C"
