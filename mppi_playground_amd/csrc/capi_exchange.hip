// capi_exchange.hip — C ABI (include/mppi_hip.h): sharded solves — the RCCL loader and the in-library collective, the
// peer-to-peer exchange of the shard summaries, and the time-out flags of the polling kernels.
#include <dlfcn.h>

#include "mppi_handle.hpp"

namespace mppi {

__global__ __launch_bounds__(BLOCK) void p2p_publish_kernel(const float* __restrict__ summary, int len, P2pCtx x) {
    const size_t slot = ((size_t)(x.seq & 1u) * x.world + x.rank) * x.lenp;
    for (int j = threadIdx.x; j < len; j += BLOCK) {
        const unsigned long long cell = cell_pack(x.seq, summary[j]);
        for (int w = 0; w < x.world; ++w) cell_store<__HIP_MEMORY_SCOPE_SYSTEM>(x.peers[w] + slot + j, cell);
    }
}

// self-test / generic use: collect into a plain device array [W][len]
__global__ __launch_bounds__(BLOCK) void p2p_collect_kernel(P2pCtx x, int len, float* __restrict__ out) {
    p2p_collect<BLOCK>(x, len, out, len);
}

// RCCL through dlopen (see RcclApi)
const RcclApi& rccl() {
    static const RcclApi api = [] {
        RcclApi a;
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return a;
        a.get_unique_id = reinterpret_cast<decltype(a.get_unique_id)>(dlsym(lib, "ncclGetUniqueId"));
        a.comm_init_rank = reinterpret_cast<decltype(a.comm_init_rank)>(dlsym(lib, "ncclCommInitRank"));
        a.comm_destroy = reinterpret_cast<decltype(a.comm_destroy)>(dlsym(lib, "ncclCommDestroy"));
        a.all_gather = reinterpret_cast<decltype(a.all_gather)>(dlsym(lib, "ncclAllGather"));
        a.error_string = reinterpret_cast<decltype(a.error_string)>(dlsym(lib, "ncclGetErrorString"));
        a.comm_count = reinterpret_cast<decltype(a.comm_count)>(dlsym(lib, "ncclCommCount"));
        a.comm_user_rank = reinterpret_cast<decltype(a.comm_user_rank)>(dlsym(lib, "ncclCommUserRank"));
        a.ok = a.get_unique_id && a.comm_init_rank && a.comm_destroy && a.all_gather && a.error_string;
        return a;
    }();
    return api;
}

}  // namespace mppi

extern "C" {

// ---- in-library collective: RCCL all_gather of the shard summaries on the solve's stream (SURVEY 8e variant A)
int mppi_comm_unique_id(void* id_out128) {
    if (!id_out128) return MPPI_E_INVALID;
    if (!rccl().ok) return MPPI_E_STATE;
    static_assert(sizeof(ncclUniqueId) == 128, "unique id size");
    return rccl().get_unique_id(reinterpret_cast<ncclUniqueId*>(id_out128)) == ncclSuccess ? MPPI_OK : MPPI_E_HIP;
}

int mppi_comm_init(mppi_handle_t h, int world, int rank, const void* id128) {
    if (!h || !id128 || world < 1 || rank < 0 || rank >= world) return fail(h, MPPI_E_INVALID, "bad comm arguments");
    if (h->xchg.comm) return fail(h, MPPI_E_STATE, "communicator already initialised");
    if (!rccl().ok) return fail(h, MPPI_E_STATE, "librccl.so.1 not found (or incomplete): no in-library collective");
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    const size_t len = (size_t)(MPPI_SUMMARY_HEAD + h->d.row);
    HIP_TRY(h, h->xchg.comm_send.alloc(len));
    HIP_TRY(h, h->xchg.comm_recv.alloc(len * (size_t)world));
    RCCL_TRY(h, rccl().comm_init_rank(&h->xchg.comm, world, id, rank));  // collective: every rank of the job calls it
    h->xchg.comm_world = world; h->xchg.comm_rank = rank;
    return MPPI_OK;
}

int mppi_comm_destroy(mppi_handle_t h) {
    if (!h) return MPPI_E_INVALID;
    h->xchg.comm_enabled = false;
    if (h->xchg.comm) { HIP_TRY(h, hipDeviceSynchronize()); (void)rccl().comm_destroy(h->xchg.comm); h->xchg.comm = nullptr; }
    return MPPI_OK;
}

// One stand-alone all_gather of data_dev [4 + T*dc] (self-test; every rank calls it the same number of times):
// gathered_out_dev [world][4 + T*dc].  Synchronises.
// What RCCL itself says about the communicator of this handle: ncclCommCount / ncclCommUserRank (diagnostics: a
// multi-GPU bench line records them next to the world size the launcher claims).
int mppi_comm_info(mppi_handle_t h, int* count_out, int* rank_out) {
    if (!h || !h->xchg.comm) return fail(h, MPPI_E_STATE, "no communicator (mppi_comm_init)");
    if (!rccl().comm_count || !rccl().comm_user_rank) return fail(h, MPPI_E_STATE, "librccl lacks ncclCommCount / ncclCommUserRank");
    int c = -1, r = -1;
    RCCL_TRY(h, rccl().comm_count(h->xchg.comm, &c));
    RCCL_TRY(h, rccl().comm_user_rank(h->xchg.comm, &r));
    if (count_out) *count_out = c;
    if (rank_out) *rank_out = r;
    return MPPI_OK;
}

int mppi_comm_exchange(mppi_handle_t h, const float* data_dev, float* gathered_out_dev, void* stream) {
    if (!h || !data_dev || !gathered_out_dev) return fail(h, MPPI_E_INVALID, "bad comm arguments");
    if (!h->xchg.comm) return fail(h, MPPI_E_STATE, "comm: not initialised");
    hipStream_t s = (hipStream_t)stream;
    RCCL_TRY(h, rccl().all_gather(data_dev, gathered_out_dev, (size_t)(MPPI_SUMMARY_HEAD + h->d.row), ncclFloat, h->xchg.comm, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    return MPPI_OK;
}

// ---- peer-to-peer exchange of the shard summaries (sharded solves; see P2pCtx in mppi_exchange.hpp)
int mppi_p2p_alloc(mppi_handle_t h, int world, int rank, void* ipc_handle_out64) {
    if (!h || !ipc_handle_out64 || world < 2 || world > 64 || rank < 0 || rank >= world)
        return fail(h, MPPI_E_INVALID, "bad p2p arguments");
    if (h->xchg.p2p_local) return fail(h, MPPI_E_STATE, "p2p buffer already allocated");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "ipc handle size");
    h->xchg.p2p_world = world; h->xchg.p2p_rank = rank;
    h->xchg.p2p_lenp = ((MPPI_SUMMARY_HEAD + h->d.row + 15) / 16) * 16;
    const size_t cells = 2 * (size_t)world * h->xchg.p2p_lenp;
    HIP_TRY(h, h->xchg.p2p_local.alloc(cells, hipDeviceMallocFinegrained));
    HIP_TRY(h, hipMemset(h->xchg.p2p_local, 0, sizeof(unsigned long long) * cells));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, h->xchg.p2p_error.alloc(1, true));
    HIP_TRY(h, hipIpcGetMemHandle(reinterpret_cast<hipIpcMemHandle_t*>(ipc_handle_out64), h->xchg.p2p_local.p));
    return MPPI_OK;
}

int mppi_p2p_connect(mppi_handle_t h, const void* ipc_handles_world_x64, const int32_t* peer_devices) {
    if (!h || !ipc_handles_world_x64 || !peer_devices) return fail(h, MPPI_E_INVALID, "bad p2p arguments");
    if (!h->xchg.p2p_local || h->xchg.p2p_connected) return fail(h, MPPI_E_STATE, "p2p: allocate first, connect once");
    // every peer GPU must be directly addressable from this one (xGMI / PCIe peer access) before any store goes out
    int ndev = 0;
    HIP_TRY(h, hipGetDeviceCount(&ndev));
    for (int w = 0; w < h->xchg.p2p_world; ++w) {
        const int pd = peer_devices[w];
        if (w == h->xchg.p2p_rank || pd == h->cfg.device) continue;
        if (pd < 0 || pd >= ndev) return fail(h, MPPI_E_STATE, "p2p: a peer's device is not visible to this process");
        int can = 0;
        HIP_TRY(h, hipDeviceCanAccessPeer(&can, h->cfg.device, pd));
        if (!can) return fail(h, MPPI_E_STATE, "p2p: no peer access to a rank's device");
    }
    std::vector<unsigned long long*> peers((size_t)h->xchg.p2p_world, nullptr);
    const hipIpcMemHandle_t* hs = reinterpret_cast<const hipIpcMemHandle_t*>(ipc_handles_world_x64);
    for (int w = 0; w < h->xchg.p2p_world; ++w) {
        if (w == h->xchg.p2p_rank) { peers[w] = h->xchg.p2p_local; continue; }
        void* pm = nullptr;
        HIP_TRY(h, hipIpcOpenMemHandle(&pm, hs[w], hipIpcMemLazyEnablePeerAccess));
        h->xchg.p2p_opened.push_back(pm);
        peers[w] = static_cast<unsigned long long*>(pm);
    }
    HIP_TRY(h, h->xchg.p2p_peers_dev.alloc((size_t)h->xchg.p2p_world));
    HIP_TRY(h, hipMemcpy(h->xchg.p2p_peers_dev, peers.data(), sizeof(unsigned long long*) * (size_t)h->xchg.p2p_world, hipMemcpyHostToDevice));
    h->xchg.p2p_connected = true;
    return MPPI_OK;
}

// One exchange of `data_dev` [4 + T*dc] outside a solve (self-test; every rank must call it the same number of
// times): gathered_out_dev [world][4 + T*dc].  Returns MPPI_E_STATE when a poll timed out.  Synchronises.
int mppi_p2p_exchange(mppi_handle_t h, const float* data_dev, float* gathered_out_dev, void* stream) {
    if (!h || !data_dev || !gathered_out_dev) return fail(h, MPPI_E_INVALID, "bad p2p arguments");
    if (!h->xchg.p2p_connected) return fail(h, MPPI_E_STATE, "p2p: not connected");
    hipStream_t s = (hipStream_t)stream;
    next_tag(h->seq.p2p);
    const int len = MPPI_SUMMARY_HEAD + h->d.row;
    hipLaunchKernelGGL(p2p_publish_kernel, dim3(1), dim3(BLOCK), 0, s, data_dev, len, p2p_ctx(h));
    hipLaunchKernelGGL(p2p_collect_kernel, dim3(1), dim3(BLOCK), 0, s, p2p_ctx(h), len, gathered_out_dev);
    HIP_TRY(h, hipGetLastError());
    HIP_TRY(h, hipStreamSynchronize(s));
    if (h->xchg.p2p_error.get()) return fail(h, MPPI_E_STATE, "p2p exchange timed out");
    return MPPI_OK;
}

// 1 once a poll of the single-launch solve timed out on this handle (read without synchronising): that solve's outputs
// are void (NaN) and the handle has returned to the multi-kernel path
#ifdef MPPI_FUSED_TRACE
extern "C" int mppi_debug_fused_trace(mppi_handle_t h, int* out10) {  // (out: 56 ints)  // 10 ns ticks since block 0 started, per phase boundary
    if (!h || !h->fused.error.host) return MPPI_E_STATE;
    (void)hipDeviceSynchronize();
    for (int k = 0; k < 24; ++k) { out10[k] = h->fused.error.host[1 + k]; h->fused.error.host[1 + k] = 0; }
    for (int k = 0; k < 32; ++k) out10[24 + k] = h->fused.error.host[32 + k];
    return MPPI_OK;
}

#endif
int mppi_fused_error(mppi_handle_t h) { return h ? h->fused.error.get() : 0; }

// grid and trajectories per block of the last mppi_solve if it ran as the single launch; 0 / 0 if it took the multi-kernel path
int mppi_fused_geometry(mppi_handle_t h, int* blocks_out, int* spb_out) {
    if (!h) return MPPI_E_INVALID;
    if (blocks_out) *blocks_out = h->fused.last_blocks;
    if (spb_out) *spb_out = h->fused.last_spb;
    return MPPI_OK;
}

// 1 if a poll of the exchange buffer ever timed out on this handle (read without synchronising)
int mppi_p2p_error(mppi_handle_t h) { return h ? h->xchg.p2p_error.get() : 0; }

}  // extern "C"
