// evpk_api.hip -- host side of libevpk: the C ABI of include/evpk.h.
//
// Mirrors the control flow of subroutine evp (source/ice_dyn_evp.F90:68-510) on one HIP
// stream: gather block arrays into the slab, evp_prep1 / to_ugrid / evp_prep2, halo
// updates, ndte x (fused stress+stepu kernel, velocity halo), tripole stress fold,
// evp_finish, u2tgrid, scatter back.  Multi-GPU: x-slabs on a ring, ghost zones of up to 8
// columns exchanged once per 4 launches with ncclSend/ncclRecv (RCCL over xGMI) beside the
// interior strips on a second stream; the tripole fold all-gathers the two top rows.
// No CPU fallback exists: every entry point needs a gfx950 device.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <fcntl.h>
#include <sched.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <mutex>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/evpk.h"
#include "evpk_internal.h"

// single translation unit: the kernels are compiled together with the host API
#include "evpk_kernels.hip"
#include "evpk_remap.hip"
#include "evpk_ridge.hip"
#include "evpk_itd.hip"
#include "evpk_therm2.hip"
#include "evpk_therm1.hip"
#include "evpk_therm1s.hip"
#include "evpk_rad.hip"
#include "evpk_dedd.hip"
#include "evpk_eap.hip"

using namespace evpk;

static thread_local std::string g_create_err;

// ------------------------------------------------------------------------------------------------------
// Rendezvous of the rank processes on a POSIX shared-memory segment.  Rank 0 replaces whatever carries the name (a crashed
// run may have left a segment behind; a previous context of this run may not have unlinked its own yet) and the other
// ranks must not trust a segment until rank 0 OF THIS RUN has answered in it: every rank > 0 writes a fresh random word
// into hello[r] of the segment it has mapped and waits for rank 0 to copy it into ack[r]; while it waits it re-opens the
// name now and then, and starts over if the name has moved on to another inode.  A stale segment is never acknowledged
// (its rank 0 is gone), so magic numbers, stages or IPC handles found in one are never read.  The last 4096 bytes of the
// segment hold the two tables.
// ------------------------------------------------------------------------------------------------------
static constexpr size_t SHM_RDV_BYTES = 4096;
static double shm_now() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static char *shm_rendezvous(const std::string &name, size_t total, int r, int n, const char *what, std::string &err) {
    const double t0 = shm_now(), limit = 120.0;
    auto hello = [&](char *b, int q) { return reinterpret_cast<uint64_t *>(b + total - SHM_RDV_BYTES) + q; };
    auto ack = [&](char *b, int q) { return reinterpret_cast<uint64_t *>(b + total - SHM_RDV_BYTES / 2) + q; };
    if ((size_t)n * 8 > SHM_RDV_BYTES / 2) { err = std::string(what) + ": too many ranks"; return nullptr; }
    if (r == 0) {
        shm_unlink(name.c_str());
        int fd = shm_open(name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
        if (fd < 0 || ftruncate(fd, (off_t)total) != 0) { if (fd >= 0) ::close(fd); err = std::string(what) + ": cannot create " + name; return nullptr; }
        char *b = (char *)mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        ::close(fd);
        if (b == MAP_FAILED) { err = std::string(what) + ": mmap failed"; return nullptr; }
        // (no memset: a segment created with O_EXCL and sized by ftruncate reads as zeros, and a rank that has already
        //  mapped it may have written its hello word)
        for (int left = n - 1; left > 0;) {
            left = 0;
            for (int q = 1; q < n; q++) {
                const uint64_t h = __atomic_load_n(hello(b, q), __ATOMIC_ACQUIRE);
                if (h) __atomic_store_n(ack(b, q), h, __ATOMIC_RELEASE); else left++;
            }
            if (left) { usleep(200); if (shm_now() - t0 > limit) { munmap(b, total); shm_unlink(name.c_str()); err = std::string(what) + ": not every rank arrived at " + name; return nullptr; } }
        }
        return b;
    }
    uint64_t nonce = ((uint64_t)getpid() << 32) ^ (uint64_t)(shm_now() * 1e9) ^ ((uint64_t)r << 56);
    for (;;) {
        if (shm_now() - t0 > limit) { err = std::string(what) + ": timeout waiting for rank 0 at " + name; return nullptr; }
        int fd = shm_open(name.c_str(), O_RDWR, 0600);
        if (fd < 0) { usleep(1000); continue; }
        struct stat st;
        if (fstat(fd, &st) != 0 || (size_t)st.st_size < total) { ::close(fd); usleep(1000); continue; }     // not sized yet (or a smaller stale one)
        const ino_t ino = st.st_ino;
        char *b = (char *)mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        ::close(fd);
        if (b == MAP_FAILED) { err = std::string(what) + ": mmap failed"; return nullptr; }
        nonce = nonce * 6364136223846793005ULL + 1442695040888963407ULL;
        if (!nonce) nonce = 1;
        __atomic_store_n(hello(b, r), nonce, __ATOMIC_RELEASE);
        bool stale = false;
        for (long k = 0; __atomic_load_n(ack(b, r), __ATOMIC_ACQUIRE) != nonce; k++) {
            usleep(200);
            if (shm_now() - t0 > limit) break;
            if ((k & 15) == 15) {          // does the name still lead to the segment I mapped?
                int fd2 = shm_open(name.c_str(), O_RDWR, 0600);
                struct stat s2;
                if (fd2 < 0 || fstat(fd2, &s2) != 0 || s2.st_ino != ino) stale = true;
                if (fd2 >= 0) ::close(fd2);
                if (stale) break;
            }
        }
        if (!stale && __atomic_load_n(ack(b, r), __ATOMIC_ACQUIRE) == nonce) return b;
        munmap(b, total);
    }
}

// ------------------------------------------------------------------------------------------------------
// Host-staged shared-memory relay: a second transport with the semantics of the RCCL point-to-point calls
// (ordered messages per (src, dst) pair), so that several ranks can run the real multi-rank code path on
// ONE GPU in tests (RCCL refuses two ranks on one device).  Selected by a unique id that starts with
// "EVPKSHM:<name>".  One mailbox of depth 1 per ordered pair in a POSIX shared-memory segment.
// ------------------------------------------------------------------------------------------------------
struct ShmRelay {
    int rank = 0, nranks = 0;
    size_t slot = 0, total = 0;
    char *base = nullptr;
    std::string name;
    std::vector<char> host;
    struct Box { uint64_t wr, rd; char pad[48]; };
    static constexpr size_t HDR = 64;
    Box *box(int src, int dst) const { return reinterpret_cast<Box *>(base + HDR + ((size_t)src * nranks + dst) * (sizeof(Box) + slot)); }
    char *payload(int src, int dst) const { return reinterpret_cast<char *>(box(src, dst)) + sizeof(Box); }
    static double now() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
    template <typename F> bool wait(F ready) const {
        const double t0 = now();
        for (long k = 0; !ready(); k++) {
            if ((k & 63) == 63) { sched_yield(); if (now() - t0 > 120.0) return false; }
        }
        return true;
    }
    int open(const std::string &nm, int r, int n, size_t slot_bytes, std::string &err) {
        rank = r; nranks = n; slot = (slot_bytes + 63) & ~size_t(63); name = "/" + nm;
        total = HDR + (size_t)n * n * (sizeof(Box) + slot);
        total = ((total + 4095) / 4096) * 4096 + SHM_RDV_BYTES;
        base = shm_rendezvous(name, total, r, n, "shm relay", err);       // (a fresh segment: every mailbox counter is 0)
        if (!base) return 1;
        host.resize(slot);
        return 0;
    }
    void close_() {
        if (base) munmap(base, total);
        base = nullptr;
        if (rank == 0 && !name.empty()) shm_unlink(name.c_str());
    }
    int send(int dst, const void *dev, size_t bytes, hipStream_t st) {
        if (bytes > slot) return 1;
        if (hipMemcpyAsync(host.data(), dev, bytes, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 1;
        Box *b = box(rank, dst);
        if (!wait([&] { return __atomic_load_n(&b->rd, __ATOMIC_ACQUIRE) == __atomic_load_n(&b->wr, __ATOMIC_RELAXED); })) return 2;
        memcpy(payload(rank, dst), host.data(), bytes);
        __atomic_store_n(&b->wr, b->wr + 1, __ATOMIC_RELEASE);
        return 0;
    }
    int recv(int src, void *dev, size_t bytes, hipStream_t st) {
        if (bytes > slot) return 1;
        Box *b = box(src, rank);
        if (!wait([&] { return __atomic_load_n(&b->wr, __ATOMIC_ACQUIRE) > __atomic_load_n(&b->rd, __ATOMIC_RELAXED); })) return 2;
        memcpy(host.data(), payload(src, rank), bytes);
        __atomic_store_n(&b->rd, b->rd + 1, __ATOMIC_RELEASE);
        if (hipMemcpyAsync(dev, host.data(), bytes, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return 1;
        return 0;
    }
};

// ------------------------------------------------------------------------------------------------------
// Peer-mapped transport (unique id "EVPKIPC:<name>"): the rank processes of ONE node map each other's receive buffers
// (hipIpcGetMemHandle / hipIpcOpenMemHandle; between GPUs the mapping goes over xGMI, between processes on one GPU it
// is the same HBM), so that a pack kernel stores straight into the neighbour's buffer and no copy engine, host thread or
// RCCL kernel sits in between.  Completion: a sequence number per ordered (src, dst) pair and channel in a page of
// page-locked host memory shared by all ranks (POSIX shared memory, hipHostRegister'ed in every process): k_ipc_signal
// behind the storing kernel, k_ipc_wait in front of the reading one.  Buffers are double buffered by the parity of the
// sequence number: every exchange of this library is a swap between the two ranks on one stream, so a rank that has
// received message k+1 knows its partner is done reading message k.  Two channels (0: `stream`, 1: `stream2`) keep the
// histories of the two streams apart.  The POSIX segment also carries the start-up data (IPC handles, slab starts).
// ------------------------------------------------------------------------------------------------------
struct IpcXp {
    static constexpr int MAXR = 16;
    int rank = 0, nranks = 0;
    std::string name;
    char *base = nullptr;
    size_t total = 0, flags_off = 0, flags_bytes = 0;
    unsigned *dflags = nullptr;              // device alias of the flag page(s)
    bool registered = false;
    char *mybox = nullptr;
    char *peer[MAXR] = {};
    size_t slot[2] = {0, 0}, chan_off[2] = {0, 0}, box_bytes = 0;
    uint32_t sent[2][MAXR] = {}, recvd[2][MAXR] = {};
    unsigned *d_err = nullptr;
    struct Info { int32_t i0; int32_t stage; char pad[56]; };
    static double now() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
    uint64_t *magic() const { return reinterpret_cast<uint64_t *>(base); }
    hipIpcMemHandle_t *handle(int r) const { return reinterpret_cast<hipIpcMemHandle_t *>(base + 64 + (size_t)r * 64); }
    Info *info(int r) const { return reinterpret_cast<Info *>(base + 64 + (size_t)nranks * 64 + (size_t)r * 64); }
    unsigned *flag(int ch, int src, int dst) const { return dflags + ((size_t)(ch * nranks + src) * nranks + dst) * 16; }
    size_t slot_off(int ch, int parity, int src) const { return chan_off[ch] + ((size_t)parity * nranks + src) * slot[ch]; }
    bool wait_stage(int stage, std::string &err) const {
        const double t0 = now();
        for (int r = 0; r < nranks; r++)
            while (__atomic_load_n(&info(r)->stage, __ATOMIC_ACQUIRE) < stage) {
                usleep(200);
                if (now() - t0 > 120.0) { err = "ipc transport: rank " + std::to_string(r) + " never reached start-up stage " + std::to_string(stage); return false; }
            }
        return true;
    }
    void set_stage(int stage) { __atomic_store_n(&info(rank)->stage, stage, __ATOMIC_RELEASE); }
    int open(const std::string &nm, int r, int n, std::string &err) {
        if (n > MAXR) { err = "ipc transport: more than 16 ranks"; return 1; }
        rank = r; nranks = n; name = "/" + nm;
        flags_off = ((64 + (size_t)n * 128 + 4095) / 4096) * 4096;
        flags_bytes = (((size_t)2 * n * n * 64 + 4095) / 4096) * 4096;
        total = flags_off + flags_bytes + SHM_RDV_BYTES;
        base = shm_rendezvous(name, total, r, n, "ipc transport", err);   // zero-filled by rank 0 of THIS run, see above
        if (!base) return 1;
        return 0;
    }
    void close_() {
        if (d_err) (void)hipFree(d_err);
        for (int q = 0; q < nranks; q++) if (q != rank && peer[q]) (void)hipIpcCloseMemHandle(peer[q]);
        if (mybox) (void)hipFree(mybox);
        if (registered) (void)hipHostUnregister(base + flags_off);
        if (base) munmap(base, total);
        base = nullptr;
        if (rank == 0 && !name.empty()) shm_unlink(name.c_str());
    }
};

struct evpk_ctx {
    Slab s{};
    DevParams p{};
    bool have_params = false, uploaded = false, prepped = false;
    bool connected = false;     // evpk_connect (or evpk_create with a unique id / one rank) has run
    bool fresh = true;          // state planes were (re)loaded from the host since the last prep
    unsigned char *tile_buf = nullptr;   // 6 tile-flag arrays: ice/dat x {A, B} (new / previous evp, swapped) + act_ice, act_any
    int tile_cur = 0;
    bool zone_mode = false;     // the pair kernels read ghost zones filled by exchange_cols (x-slabs / forced exchange)
    // Ghost zones are zW = 2*zM columns wide (2*zM + 1 when the tripole band runs between ranks: evpk_connect): a two-subcycle launch consumes two columns of validity per side, the zone
    // columns themselves are advanced redundantly, so the neighbours exchange once per zM launches (communication avoiding).
    int zW = 2, zM = 1;
    int zone_left = 0;          // launches the zones of the current state buffer are still good for
    bool inner_ok = false;      // ghost columns 0 / nxl+1 (u, v, sigma) of the current state buffer are valid
    bool zcompact = false;      // state exchanges carry only the rows with an active cell in the zone window
    unsigned char *d_zflags = nullptr;
    int *d_zrows = nullptr;     // 4 row lists (send W, send E, recv E, recv W), nyl+2 ints each
    int zn[4] = {0, 0, 0, 0};
    // ice_strength on the device (evpk_step_in.strength == NULL)
    bool strength_dev = false;
    double *itd = nullptr;            // 2*ncat+1 plain planes: aicen, vicen, aice0
    double *stage_itd = nullptr;      // staging of one (nx_block, ny_block, ncat, nblocks) host array
    int itd_ncat = 0;
    bool zone_metrics_done = false;   // the time-invariant planes of the zones have been exchanged
    int zone_exchanges = 0;     // in the last evpk_subcycle call
    long long zone_bytes = 0;
    hipEvent_t evE = nullptr;   // after the most recent kernel launch on `stream`
    hipEvent_t evB0 = nullptr, evB1 = nullptr;   // tripole, single rank: band 1 + its fold on stream2 beside the main launch
    // EVPK_HANDOVER=value: the two hand-overs of a pair through stream memory operations on signal memory (hipStreamWriteValue32 /
    // hipStreamWaitValue32) instead of an event record + wait pair: ~5 us per pair cheaper (3600x2700 tripole 14.87 -> 14.53 ms, 1440x1080
    // 4.34 -> 4.03), bit-identical -- but NOT the default: a queue blocked in a value wait deadlocks under rocprofv3 --pmc (the
    // counter passes serialise the dispatches of all queues), and starves partner ranks that share a device
    uint32_t *sigB = nullptr, *sigB1 = nullptr;  // pairs the main stream has completed / band sequences stream2 has completed (8 bytes each)
    uint32_t sig_seq = 0;
    bool handover_value = false;
    int nxb = 0, nyb = 0, nblocks = 0;
    std::vector<BlockDesc> bd;
    BlockDesc *d_bd = nullptr;
    bool full_cover = true;
    bool band_fused = true;       // EVPK_BAND_FUSED (default 1): see subcycle_impl
    // x-slab ranks on a tripole grid (even number of ranks, equal slab widths; EVPK_XBAND=0: band launches on the second stream):
    // the mirror slab M of band_pair -- a copy of rows N-3 .. N+1 of the mirror rank P-1-r (its ghost zones included), kept
    // current by one row message per pair (rows N-3, N-2; all five after a ghost-zone exchange or a one-subcycle launch)
    bool xband = false;
    Slab m{};
    Slab *d_mslab = nullptr;
    double2 *xb_send = nullptr, *xb_recv = nullptr;
    size_t xb_cap = 0;
    int w_bound = 0;
    bool xb_fuse = true, xb_merge = true;
    bool finish_fused = true;     // EVPK_FINISH_FUSED=0: k_finish, halo, k_to_tgrid2 on one rank as well
    int m_need = 1, xb_swaps = 0;     // m_need: the mirror slab's state must be fetched before the next pair launch
    struct XbPeer { int rank; XbSeg seg; };
    std::vector<XbPeer> xb_to, xb_from;   // whose mirror slabs hold columns of mine (runs of MY columns); who holds columns of my M (runs of M's)
    int *d_mstrips = nullptr;        // every strip of the mirror slab (its own advance between two refreshes), for (ms_R, ms_ncx)
    int ms_R = 0, ms_ncx = 0, ms_n = 0;
    // strip list of the pair kernels compacted on the device (one rank, no ghost zones; EVPK_DEVICE_STRIPS=0: on the host):
    // evpk_prep then never waits for the GPU -- the kernels read the list's length from d_ns2, the host reads it (and the cell
    // counts) from page-locked memory once the loop's final event has completed
    bool dev_strips_env = true, dev_strips = false;
    bool counts_pending = false;      // dev_strips: icellt / icellu / nstrips2 of this evp are still on their way into h_counts
    int *d_ns2 = nullptr;
    unsigned long long *h_counts = nullptr;      // page-locked: [0] icellt, [1] icellu, [2] number of strips (as written by the copies)
    int ns_tot2_cur = 0;
    int ew = 0, ns = 0, rank = 0, nranks = 1, west = -1, east = -1, device = 0;
    // nranks is the RING: the ranks that own block columns (create_distrb_cart gives rank r the block columns r*nbx_pp+1 ..
    // (r+1)*nbx_pp with nbx_pp = ceil(nblocks_x / nprocs): the last ranks may get none, ice_distribution.F90:603-640).  xranks is
    // the host's count, the size of the transport's world.  An idle rank (rank >= nranks) joins evpk_connect -- the communicator /
    // the start-up stages of the peer-mapped transport are collective over the host's ranks -- and every other call returns at
    // once: it has no slab, nobody's ghost zone or mirror slab holds a column of it, so it is in no exchange.
    int xranks = 1;
    bool idle = false;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;   // interior strips of the pair kernel while `stream` exchanges the edge columns
    hipEvent_t evI = nullptr, evX = nullptr;
    int *d_strips2e = nullptr, *d_strips2i = nullptr;
    int *d_band = nullptr;           // strips 0..ncx-1 of a one-band launch (tripole top band)
    bool strips1_valid = false;      // d_strips / nstrips (one-subcycle kernel) match the masks of the last prep
    bool band_mode = false;          // tripole + pair kernels: the top rows are redone with two one-subcycle band launches
    int nstrips2e = 0, nstrips2i = 0;
    bool overlap = true;
    bool ov_fixed = true;            // false: still trying the split against whole launches (first three evps on x-slabs)
    int ov_trial = 0;
    float ov_ms[2] = {0.f, 0.f};     // loop time with the split on / off
    bool compact = false;           // k_subcycle2p reads HTN/HTE instead of the eight metric planes (verified at create)
    ncclComm_t comm = nullptr;
    ShmRelay *relay = nullptr;      // test transport instead of RCCL (unique id "EVPKSHM:<name>")
    IpcXp *ipc = nullptr;           // peer-mapped transport (unique id "EVPKIPC:<name>")
    // tripole fold between x-slab ranks: who needs this rank's top rows, whose rows this rank needs (mirror ranks)
    std::vector<int> fold_dst, fold_src;
    double *foldseg = nullptr;      // this rank's own segment (it is its own fold partner too) / local send buffer
    double *foldrcv = nullptr;      // receive buffers, one segment of wmax columns per source rank (transports without mapped buffers)
    double *stage = nullptr;   // nblocks*nyb*nxb doubles (also reused as int32)
    size_t stage_n = 0;
    // strips
    int ncx = 0, nry = 0, R = 8, nstrips = 0;
    int ncx2 = 0, nstrips2 = 0;      // 61-column strips of the two-subcycle kernel
    int R2 = 16, nry2 = 0;           // their height, tuned to the active area (tune_R2)
    long long tuned_icellt = -1, tuned1_icellt = -1;
    int slots2 = 512;                // resident 256-thread workgroups of k_subcycle2p on the whole chip
    int nsimd = 1024;                // SIMDs of the chip (4 per CU)
    double *tp_a = nullptr, *tp_b = nullptr;              // transport_upwind: two scratch planes
    // the pool the caller's pageable arrays of one call are staged into (stage_in): call_stage for a single entry point, dyn_stage for
    // evpk_step_dynamics, which holds it across the entry points it calls
    double *call_stage = nullptr, *dyn_stage = nullptr; size_t call_stage_n = 0, dyn_stage_n = 0;
    // transport_remap: grid planes (dxu, dyu, hm), the plane pool of one call shape, its pointer tables, the error word
    double *rm_grid = nullptr, *rm_pool = nullptr;
    double **rm_tab = nullptr;
    signed char *rm_sgn = nullptr;
    unsigned *rm_bad = nullptr;
    int *d_bmap = nullptr; int bmap_nbx = 0;              // remap_block_map
    double *uw_pool = nullptr; size_t uw_pool_n = 0;      // evpk_transport_upwind_state: one input + 3 + ntrcr output planes
    double **uw_tab = nullptr; signed char *uw_sgn = nullptr;
    size_t rm_pool_n = 0, rm_tab_n = 0, rm_sgn_n = 0;
    // evpk_ridge_ice: the planes that pass between its kernels, the ridging masks, the per-iteration block flags, the control words
    double *rg_pool = nullptr;
    unsigned *rg_mask = nullptr;
    int *rg_flags = nullptr;
    RidgeCtl *rg_ctl = nullptr;
    size_t rg_pool_n = 0, rg_mask_n = 0, rg_flags_n = 0;
    // evpk_cleanup_itd: the per-block masks of the boundaries at which a block shifts, the stop key
    unsigned *itd_bmask = nullptr; size_t itd_bmask_n = 0;
    unsigned long long *itd_key = nullptr;
    // evpk_step_therm1: the per-category planes of atmo_boundary_layer (eight) and fbot, Tbot where the caller does not ask for them
    double *th1_pool = nullptr; size_t th1_pool_n = 0;
    // evpk_bound_state: whether the blocks are the uniform tiling k_bound_state's block table assumes (0 not looked at yet, 1 yes, -1 no)
    int bs_uniform = 0;
    // ... on x-slab ranks (itd_bound_ranks): local message buffers of the transports without mapped slots, [send | recv] per partner;
    // rounds and planes of the last bound_state (evpk_stats)
    double *br_buf = nullptr; size_t br_buf_n = 0;
    int bs_rounds = 0, bs_planes = 0;
    // evpk_step_dynamics: check_only makes the stage routines return after their argument checks, before the first copy or launch
    bool check_only = false;
    // EAP (kdyn = 2): set by evpk_eap_init -- the subcycle loop then runs stress_eap / stepu / stepa (evpk_eap.hip)
    bool eap = false;
    EapDev E{};
    double *eap_pool = nullptr, *eap_tab = nullptr;
    bool have_lengths = false;       // HTN / HTE were given in evpk_geom
    unsigned char *io_raw = nullptr, *io_act = nullptr;   // sparse I/O: tiles whose inputs are uploaded this step
    long long evp_count = 0;         // evpk_prep calls so far
    long long last_dl[F_COUNT] = {};  // evp_count at which each field was last downloaded (state fields under their F_STATE0 ids)
    bool io_sparse_now = false;      // the last evpk_upload was a sparse one: evpk_download may skip inactive tiles too
    bool tile_mode = false;          // the pairs run k_subcycle2t (one row per wave, no march): chosen by tune_R2 when strips are scarce
    int tile_force = -1;             // EVPK_TILE=0 / 1 fixes the choice (2 asked for the rolling tile kernel of round 5: retired, refused)
    unsigned int *d_tune = nullptr;
    bool use_double = false;
    unsigned char *d_flags2 = nullptr;
    int *d_strips2 = nullptr;
    int double_launches = 0;
    int prio = 1;                        // EVPK_PRIO (default 1): SubArgs.prio
    int band_last = 1;                   // EVPK_BAND_LAST (default 1): SubArgs.band_last
    unsigned char *up_dat = nullptr;     // per tile: the uploaded inputs hold something (k_up_tiles)
    bool up_dirty = true;                // ... and an upload has happened since it was computed
    const char *dbg_file = nullptr;      // EVPK_DEBUG_CLOCKS
    unsigned long long *d_dbg = nullptr;
    unsigned char *d_flags = nullptr;
    int *d_strips = nullptr;
    unsigned long long *d_counts = nullptr;
    long long icellt = 0, icellu = 0;
    // exchange
    int max_nf = NSTATE;
    double *sendbuf = nullptr, *recvbuf = nullptr;   // [W edge | E edge] and [from east | from west]
    double *sendW = nullptr, *sendE = nullptr, *recvW = nullptr, *recvE = nullptr;
    double *foldbuf = nullptr, *foldloc = nullptr, *foldall = nullptr;
    double2 *cbuf = nullptr;         // 4 x [25 planes][rows][8 cols] of double2: sendW, sendE, recvE, recvW
    size_t cslot = 0;
    int wmax = 0;
    std::vector<int> slab_i0;   // nranks+1 global start columns
    int *d_slab_i0 = nullptr;
    int cur = 0, ksub = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> kev;
    float loop_ms = 0.f, kernel_ms = 0.f, kernel2_ms = 0.f;
    int kernel_launches = 0, kernel_timed = 0, kernel2_timed = 0;
    std::vector<hipEvent_t> bev;   // event pairs around sampled halo / fold / ghost-zone updates of the subcycle loop (timer_bound)
    int bound_updates = 0, bound_timed = 0;
    float bound_ms = 0.f;
    std::vector<int> kev_kind, kev_count;   // per timed span: subcycles per launch of its kernels (1, 2, 3), launches inside it
    int time_kernels = 1;          // EVPK_TIME_KERNELS: 0 none, 1 HIP events around launches 3..8 of every 20 (default), 2 every launch
    int nkev = 0;
    // EVPK_VERIFY_DELIVERY (diagnostic): every plane a download writes IN PLACE into a caller's page-locked array is delivered a second
    // time through the staging buffer + hipMemcpy and the two are compared on the host, value for value.  1: a difference is an error
    // that names plane, block, cell and 4-KiB page; 2: the caller's array is repaired from the staged copy and the event counted
    bool xfer_fused = true;        // EVPK_XFER_FUSED=0: one gather / scatter launch per array instead of up to XFER_MAX arrays per launch
    int verify_delivery = 0;
    long long dv_checked = 0, dv_bad = 0, dv_planes = 0;
    std::vector<double> dv_host;
    bool force_exchange = false;   // EVPK_FORCE_EXCHANGE=1: single rank takes the multi-rank pack/exchange/unpack path (tests)
    std::string err;
};

#define FAIL(c, ...)                                   \
    do {                                               \
        char _b[512];                                  \
        snprintf(_b, sizeof(_b), __VA_ARGS__);         \
        (c)->err = _b;                                 \
        return 1;                                      \
    } while (0)

#define HIPCHK(c, call)                                                                          \
    do {                                                                                         \
        hipError_t _e = (call);                                                                  \
        if (_e != hipSuccess) FAIL(c, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// a launch with one grid layer per local block: none when a rank has no block (grid dimension 0 is not a launch)
#define LAUNCH_BLOCKS(kern, g, b, shm, st, ...) do { if ((g).z) hipLaunchKernelGGL(kern, g, b, shm, st, __VA_ARGS__); } while (0)

#define NCCLCHK(c, call)                                                                         \
    do {                                                                                         \
        ncclResult_t _e = (call);                                                                \
        if (_e != ncclSuccess) FAIL(c, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

static inline dim3 grid2d(const Slab &s, dim3 b) { return dim3((s.nxl + 2 + b.x - 1) / b.x, (s.nyl + 2 + b.y - 1) / b.y); }
static const dim3 B2D(64, 4);

extern "C" int evpk_slab_layout(int32_t nx_global, int32_t nranks, int32_t rank, int32_t ew_boundary,
                                int32_t i0, int32_t i1, int32_t out[5]) {
    if (nranks < 1 || rank < 0 || rank >= nranks || i1 < i0 || i0 < 1 || i1 > nx_global) return 1;
    int west = rank - 1, east = rank + 1;
    if (west < 0) west = (ew_boundary == EVPK_BND_CYCLIC) ? nranks - 1 : -1;
    if (east >= nranks) east = (ew_boundary == EVPK_BND_CYCLIC) ? 0 : -1;
    if (nranks == 1) { west = east = (ew_boundary == EVPK_BND_CYCLIC) ? 0 : -1; }
    out[0] = west; out[1] = east; out[2] = i0; out[3] = i1;
    out[4] = (nx_global + nranks - 1) / nranks;
    return 0;
}

extern "C" int evpk_get_unique_id(void *id) {
    static_assert(sizeof(ncclUniqueId) <= EVPK_UNIQUE_ID_BYTES, "unique id size");
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return 1;
    memset(id, 0, EVPK_UNIQUE_ID_BYTES);
    memcpy(id, &u, sizeof(u));
    return 0;
}

extern "C" const char *evpk_last_error(const evpk_ctx *c) { return c ? c->err.c_str() : g_create_err.c_str(); }

// ---- page-locked host arrays -------------------------------------------------------------
// A host array registered with evpk_pin_host is read / written IN PLACE by the gather / scatter kernels over PCIe
// (zero copy): no staging copy, and a download touches only the cells it delivers, so the round trip that keeps the
// caller's other cells is not needed.  Unregistered arrays take the staged path below.
//
// The library keeps its OWN table of what it may touch in place (round 5): an array is read / written through its device
// alias only if the whole of it lies inside a range that evpk_pin_host registered (and evpk_unpin_host has not released)
// or that evpk_host_alloc handed out -- never because the HIP runtime happens to know the address from some other
// registration (a stale one that overlaps a recycled heap address would otherwise silently take the zero-copy path).
// A registered range is hardened as far as an unprivileged process can: MADV_NOHUGEPAGE on its pages (no khugepaged
// collapse of the heap pages under an in-flight kernel) and mlock (best effort).  hipHostRegister'ed memory is mirrored by
// the driver through MMU notifiers, not hard-pinned: memory that must never move comes from evpk_host_alloc
// (hipHostMalloc: allocated and pinned by the driver).  EVPK_PIN_HARDEN=0 skips the two advisories.
struct PinRange {
    uintptr_t lo = 0, hi = 0;       // [lo, hi) as registered
    char *dev = nullptr;            // device alias of lo
    bool owned = false;             // evpk_host_alloc
    bool locked = false;            // mlock succeeded on its pages
};
static std::mutex g_pin_mu;
static std::vector<PinRange> g_pins;
static long g_page = 0;
static inline uintptr_t page_lo(uintptr_t a) { return a & ~(uintptr_t)(g_page - 1); }
static inline uintptr_t page_hi(uintptr_t a) { return (a + g_page - 1) & ~(uintptr_t)(g_page - 1); }

extern "C" int evpk_pin_host(void *ptr, size_t bytes) {
    if (!ptr || !bytes) return 1;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (!g_page) g_page = sysconf(_SC_PAGESIZE) > 0 ? sysconf(_SC_PAGESIZE) : 4096;
    const uintptr_t lo = (uintptr_t)ptr, hi = lo + bytes;
    for (const PinRange &r : g_pins)
        if (lo < r.hi && r.lo < hi) return 1;           // overlaps a live registration: refuse (unpin first)
    PinRange r;
    r.lo = lo; r.hi = hi;
    const char *hard = getenv("EVPK_PIN_HARDEN");
    if (!hard || atoi(hard) != 0) {
        const uintptr_t pl = page_lo(lo), ph = page_hi(hi);
        (void)madvise((void *)pl, ph - pl, MADV_NOHUGEPAGE);
        r.locked = (mlock((void *)pl, ph - pl) == 0);
    }
    hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    void *dp = nullptr;
    if (e == hipSuccess) {
        e = hipHostGetDevicePointer(&dp, ptr, 0);
        if (e != hipSuccess) (void)hipHostUnregister(ptr);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (r.locked) (void)munlock((void *)page_lo(lo), page_hi(hi) - page_lo(lo));
        return 1;
    }
    r.dev = (char *)dp;
    g_pins.push_back(r);
    return 0;
}

extern "C" int evpk_unpin_host(void *ptr) {
    if (!ptr) return 1;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t k = 0; k < g_pins.size(); k++) {
        if (g_pins[k].lo != (uintptr_t)ptr || g_pins[k].owned) continue;
        const PinRange r = g_pins[k];
        g_pins.erase(g_pins.begin() + k);
        const hipError_t e = hipHostUnregister(ptr);
        if (e != hipSuccess) (void)hipGetLastError();
        if (r.locked) {
            // pages shared with another live registration (heap arrays are not page aligned) stay locked
            uintptr_t pl = page_lo(r.lo), ph = page_hi(r.hi);
            for (const PinRange &o : g_pins) {
                if (o.owned) continue;
                if (page_hi(o.hi) > pl && page_lo(o.lo) <= pl) pl = std::min(ph, page_hi(o.hi));
                if (page_lo(o.lo) < ph && page_hi(o.hi) >= ph) ph = std::max(pl, page_lo(o.lo));
            }
            if (ph > pl) (void)munlock((void *)pl, ph - pl);
        }
        return e == hipSuccess ? 0 : 1;
    }
    return 1;       // not a range evpk_pin_host registered
}

// Page-locked host memory allocated AND pinned by the driver (hipHostMalloc), mapped into the device address space: the
// home for arrays of a host model that can choose where they live (allocatable module arrays, the Python mirror's fields).
// Such memory cannot migrate, be collapsed into huge pages or be swapped under a kernel that reads / writes it in place.
extern "C" int evpk_host_alloc(size_t bytes, void **out) {
    if (!out || !bytes) return 1;
    *out = nullptr;
    void *p = nullptr, *dp = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return 1; }
    if (hipHostGetDevicePointer(&dp, p, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(p); return 1; }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    PinRange r;
    r.lo = (uintptr_t)p; r.hi = r.lo + bytes; r.dev = (char *)dp; r.owned = true;
    g_pins.push_back(r);
    *out = p;
    return 0;
}

extern "C" int evpk_host_free(void *ptr) {
    if (!ptr) return 1;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (size_t k = 0; k < g_pins.size(); k++) {
        if (g_pins[k].lo != (uintptr_t)ptr || !g_pins[k].owned) continue;
        g_pins.erase(g_pins.begin() + k);
        if (hipHostFree(ptr) != hipSuccess) { (void)hipGetLastError(); return 1; }
        return 0;
    }
    return 1;
}

// 1 if [ptr, ptr + bytes) lies inside a live evpk_pin_host / evpk_host_alloc range (the library will move it in place), else 0
extern "C" int evpk_host_is_mapped(const void *ptr, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    const uintptr_t lo = (uintptr_t)ptr, hi = lo + bytes;
    for (const PinRange &r : g_pins)
        if (lo >= r.lo && hi <= r.hi) return 1;
    return 0;
}

// device-visible alias of a host array the library registered or allocated -- or the pointer itself if the caller's array
// already lives in device memory (a host model that keeps its fields on the GPU: OpenMP target / OpenACC `use_device`
// data) -- else nullptr: the staged path
static void *mapped_alias(const void *host, size_t bytes, bool *host_in_place = nullptr) {
    if (host_in_place) *host_in_place = false;
    if (!host) return nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        const uintptr_t lo = (uintptr_t)host, hi = lo + bytes;
        for (const PinRange &r : g_pins)
            if (lo >= r.lo && hi <= r.hi) {      // (the alias of registered memory usually IS the host address: unified addressing)
                if (host_in_place) *host_in_place = true;
                return r.dev + (lo - r.lo);
            }
    }
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, host) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (at.type == hipMemoryTypeDevice) return const_cast<void *>(host);
    return nullptr;
}

// a device buffer of the context that only grows: at least `need` elements behind p afterwards (n counts them); a new buffer loses the
// old contents and is zeroed on c->stream if asked
template <class T> static hipError_t grow(evpk_ctx *c, T *&p, size_t &n, size_t need, bool zero = false) {
    if (n >= need) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; n = 0;
    const hipError_t e = hipMalloc(&p, sizeof(T) * need);
    if (e != hipSuccess) return e;
    n = need;
    return zero ? hipMemsetAsync(p, 0, sizeof(T) * need, c->stream) : hipSuccess;
}

// the caller's arrays of one call: in place where the device sees them (mapped_alias, array by array), else through a staging copy -- up
// into one pool, and down again at the end if the array is an output.  A NULL or empty array gets a null device pointer.  in = false: an
// array the call writes on every element before it reads it -- it gets its place in the pool and is not copied up.  An OptArr is a HostArr
// the caller may leave NULL; any_missing answers for the others, on the list that stage_in gets.
struct HostArr {
    void *host; size_t bytes; void **slot; bool out; bool in; bool staged = false, required = true;
    template <class T, class U> HostArr(T *h, size_t count, U **dev, bool o, bool i = true)
        : host((void *)h), bytes(sizeof(T) * count), slot((void **)dev), out(o), in(i) {}
};
struct OptArr : HostArr {
    template <class... A> OptArr(A... a) : HostArr(a...) { required = false; }
};
static bool any_missing(const std::vector<HostArr> &arr) {
    return std::any_of(arr.begin(), arr.end(), [](const HostArr &a) { return a.required && !a.host; });
}
// (the upward copies are asynchronous on c->stream: the caller synchronises once, with whatever else it sends from pageable memory)
static int stage_in(evpk_ctx *c, std::vector<HostArr> &arr, bool dyn = false) {
    size_t need = 0;
    for (HostArr &a : arr) {
        *a.slot = (a.host && a.bytes) ? mapped_alias(a.host, a.bytes) : nullptr;
        a.staged = a.host && a.bytes && !*a.slot;
        if (a.staged) need += (a.bytes + 7) / 8;
    }
    double *&pool = dyn ? c->dyn_stage : c->call_stage;
    HIPCHK(c, grow(c, pool, dyn ? c->dyn_stage_n : c->call_stage_n, need));
    double *q = pool;
    for (HostArr &a : arr)
        if (a.staged) {
            if (a.in) HIPCHK(c, hipMemcpyAsync(q, a.host, a.bytes, hipMemcpyHostToDevice, c->stream));
            *a.slot = q; q += (a.bytes + 7) / 8;
        }
    return 0;
}
// the outputs back to the caller and the one synchronisation that ends a call
static int stage_out(evpk_ctx *c, const std::vector<HostArr> &arr) {
    for (const HostArr &a : arr)
        if (a.staged && a.out) HIPCHK(c, hipMemcpyAsync(a.host, *a.slot, a.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- host<->device transfer of one field -------------------------------------------------
// (asynchronous on c->stream; evpk_upload / evpk_download synchronise once at their end)
static int upload_f(evpk_ctx *c, const double *host, int f, const unsigned char *act = nullptr);
static int upload_f(evpk_ctx *c, const double *host, int f, const unsigned char *act) {
    if (!host || !c->nblocks) return 0;
    const size_t n = (size_t)c->nblocks * c->nyb * c->nxb;
    const double *src = (const double *)mapped_alias(host, n * sizeof(double));
    if (!src) {
        HIPCHK(c, hipMemcpyAsync(c->stage, host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        src = c->stage;
    }
    if (!c->full_cover) hipLaunchKernelGGL(k_fill_plane, grid2d(c->s, B2D), B2D, 0, c->stream, c->s, f, 0.0);
    dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
    LAUNCH_BLOCKS(k_gather_f, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, src, f, act);
    HIPCHK(c, hipGetLastError());
    return 0;
}

static int upload_m(evpk_ctx *c, const int32_t *host, int32_t *dev_plane) {
    if (!host || !c->nblocks) return 0;
    const size_t n = (size_t)c->nblocks * c->nyb * c->nxb;
    const int32_t *src = (const int32_t *)mapped_alias(host, n * sizeof(int32_t));
    if (!src) {
        HIPCHK(c, hipMemcpyAsync(c->stage, host, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        src = (const int32_t *)c->stage;
    }
    if (!c->full_cover) HIPCHK(c, hipMemsetAsync(dev_plane, 0, mask_elems(c->s) * sizeof(int32_t), c->stream));
    dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
    LAUNCH_BLOCKS(k_gather_m, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, src, dev_plane);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// EVPK_VERIFY_DELIVERY: c->stage holds the sentinel everywhere except where the scatter kernel of this plane has just written the
// values it ALSO wrote in place into the caller's page-locked array `host`; fetch it with a plain copy, wait for both, compare.
static constexpr uint32_t DV_SENTINEL32 = 0x7ff4a5a5u;      // (as a pair of words: a signalling NaN no kernel of this library produces)
static int verify_plane(evpk_ctx *c, void *host, size_t elem, size_t n, int f, const char *kind) {
    c->dv_host.resize((n * elem + 7) / 8);
    HIPCHK(c, hipMemcpyAsync(c->dv_host.data(), c->stage, n * elem, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t nblk = (size_t)c->nyb * c->nxb;
    long long bad = 0, seen = 0;
    size_t first = 0;
    if (const char *inj = getenv("EVPK_VERIFY_INJECT")) {
        // test hook: plane number <inj> of this context's checked planes "loses" the in-place write of its first delivered value
        if (atoll(inj) == c->dv_planes) {
            for (size_t k = 0; k < n; k++) {
                const bool del = elem == 8 ? reinterpret_cast<const uint64_t *>(c->dv_host.data())[k] != (((uint64_t)DV_SENTINEL32 << 32) | DV_SENTINEL32)
                                           : reinterpret_cast<const uint32_t *>(c->dv_host.data())[k] != DV_SENTINEL32;
                if (!del) continue;
                if (elem == 8) reinterpret_cast<uint64_t *>(host)[k] ^= 0x7ull; else reinterpret_cast<uint32_t *>(host)[k] ^= 0x7u;
                break;
            }
        }
    }
    c->dv_planes++;
    auto differs = [&](size_t k) -> bool {
        if (elem == 8) {
            const uint64_t d = reinterpret_cast<const uint64_t *>(c->dv_host.data())[k];
            if (d == (((uint64_t)DV_SENTINEL32 << 32) | DV_SENTINEL32)) return false;
            seen++;
            return d != reinterpret_cast<const volatile uint64_t *>(host)[k];
        }
        const uint32_t d = reinterpret_cast<const uint32_t *>(c->dv_host.data())[k];
        if (d == DV_SENTINEL32) return false;
        seen++;
        return d != reinterpret_cast<const volatile uint32_t *>(host)[k];
    };
    for (size_t k = 0; k < n; k++)
        if (differs(k)) { if (!bad++) first = k; }
    c->dv_checked += seen;
    if (!bad) return 0;
    c->dv_bad += bad;
    const size_t blk = first / nblk, j = (first % nblk) / c->nxb + 1, i = first % c->nxb + 1;
    const uintptr_t addr = (uintptr_t)host + first * elem;
    char msg[400];
    if (elem == 8) {
        const double hv = reinterpret_cast<const double *>(host)[first], dv = c->dv_host[first];
        snprintf(msg, sizeof(msg), "delivery check: %s %d, block %zu, (i,j) = (%zu,%zu), host address %#lx (4-KiB page %#lx): the caller's page-locked array "
                 "holds %.17g, the device delivered %.17g; %lld of %lld delivered values of the plane differ", kind, f, blk + 1, i, j,
                 (unsigned long)addr, (unsigned long)(addr >> 12), hv, dv, bad, seen);
    } else {
        snprintf(msg, sizeof(msg), "delivery check: %s plane, block %zu, (i,j) = (%zu,%zu), host address %#lx (4-KiB page %#lx): the caller's page-locked array "
                 "holds %d, the device delivered %d; %lld of %lld delivered values differ", kind, blk + 1, i, j, (unsigned long)addr,
                 (unsigned long)(addr >> 12), reinterpret_cast<const int32_t *>(host)[first], reinterpret_cast<const int32_t *>(c->dv_host.data())[first], bad, seen);
    }
    if (const char *log = getenv("EVPK_VERIFY_LOG")) {
        // the whole picture of the event, for the record: which elements, where in their pages, what the kernel's memory counters say
        if (FILE *fp = fopen(log, "a")) {
            fprintf(fp, "%s\n", msg);
            fprintf(fp, "  array base %#lx (page offset %lu), %zu elements of %zu bytes; differing elements (index: byte offset in its 4-KiB page, host | device):\n",
                    (unsigned long)(uintptr_t)host, (unsigned long)((uintptr_t)host & 4095), n, elem);
            long long shown = 0;
            size_t run0 = 0, prev = 0;
            bool inrun = false;
            for (size_t k = 0; k < n; k++) {
                bool d;
                if (elem == 8) {
                    const uint64_t dv = reinterpret_cast<const uint64_t *>(c->dv_host.data())[k];
                    d = dv != (((uint64_t)DV_SENTINEL32 << 32) | DV_SENTINEL32) && dv != reinterpret_cast<const volatile uint64_t *>(host)[k];
                    if (d && shown < 48) {
                        fprintf(fp, "    %zu: +%lu  %.17g | %.17g\n", k, (unsigned long)(((uintptr_t)host + k * 8) & 4095), reinterpret_cast<const double *>(host)[k], c->dv_host[k]);
                        shown++;
                    }
                } else {
                    const uint32_t dv = reinterpret_cast<const uint32_t *>(c->dv_host.data())[k];
                    d = dv != DV_SENTINEL32 && dv != reinterpret_cast<const volatile uint32_t *>(host)[k];
                }
                if (d) { if (!inrun) { run0 = k; inrun = true; } prev = k; }
                else if (inrun && k > prev + 64) { fprintf(fp, "    span %zu .. %zu (%zu elements, pages %#lx .. %#lx)\n", run0, prev, prev - run0 + 1,
                                                         (unsigned long)(((uintptr_t)host + run0 * elem) >> 12), (unsigned long)(((uintptr_t)host + prev * elem) >> 12)); inrun = false; }
            }
            if (inrun) fprintf(fp, "    span %zu .. %zu (%zu elements, pages %#lx .. %#lx)\n", run0, prev, prev - run0 + 1,
                               (unsigned long)(((uintptr_t)host + run0 * elem) >> 12), (unsigned long)(((uintptr_t)host + prev * elem) >> 12));
            if (FILE *vm = fopen("/proc/vmstat", "r")) {
                char line[128];
                fprintf(fp, "  vmstat:");
                while (fgets(line, sizeof(line), vm))
                    if (!strncmp(line, "thp_", 4) || !strncmp(line, "numa_", 5) || !strncmp(line, "pgmigrate", 9) || !strncmp(line, "compact_migrate", 15)) {
                        line[strcspn(line, "\n")] = 0;
                        fprintf(fp, " %s;", line);
                    }
                fclose(vm);
                fprintf(fp, "\n");
            }
            fclose(fp);
        }
    }
    if (c->verify_delivery >= 2) {      // repair: the staged copy is the device's word
        for (size_t k = 0; k < n; k++) {
            if (elem == 8) {
                const uint64_t d = reinterpret_cast<const uint64_t *>(c->dv_host.data())[k];
                if (d != (((uint64_t)DV_SENTINEL32 << 32) | DV_SENTINEL32)) reinterpret_cast<uint64_t *>(host)[k] = d;
            } else {
                const uint32_t d = reinterpret_cast<const uint32_t *>(c->dv_host.data())[k];
                if (d != DV_SENTINEL32) reinterpret_cast<uint32_t *>(host)[k] = d;
            }
        }
        return 0;
    }
    c->err = msg;
    return 1;
}

// ---- several arrays per launch (k_gather_multi / k_scatter_multi): arrays the device sees in place are collected, the others go one
// by one through the staging buffer as before.  EVPK_XFER_FUSED=0: one launch per array everywhere
struct XferBatch {
    evpk_ctx *c;
    XferList L{};
    const unsigned char *act = nullptr;
    bool up = true;
    int flush() {
        if (!L.n) return 0;
        const dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
        if (up) LAUNCH_BLOCKS(k_gather_multi, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, L, act);
        else LAUNCH_BLOCKS(k_scatter_multi, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, L, act);
        L.n = 0;
        HIPCHK(c, hipGetLastError());
        return 0;
    }
};
static int upload_f(evpk_ctx *c, const double *host, int f, const unsigned char *act);
// upload of one field through the batch when its array is visible to the device, else at once through the staging buffer
static int upload_fb(XferBatch &B, const double *host, int f, const unsigned char *act) {
    evpk_ctx *c = B.c;
    if (!host || !c->nblocks) return 0;
    const size_t n = (size_t)c->nblocks * c->nyb * c->nxb;
    double *src = c->xfer_fused ? (double *)mapped_alias(host, n * sizeof(double)) : nullptr;
    if (!src) return upload_f(c, host, f, act);
    if (B.L.n && (B.act != act || B.L.n == XFER_MAX)) { if (B.flush()) return 1; }
    if (!c->full_cover) hipLaunchKernelGGL(k_fill_plane, grid2d(c->s, B2D), B2D, 0, c->stream, c->s, f, 0.0);
    B.act = act; B.up = true;
    B.L.f[B.L.n] = f; B.L.mode[B.L.n] = 0; B.L.host[B.L.n] = src; B.L.n++;
    return 0;
}

// staged downloads start from the caller's bytes so that cells the reference leaves untouched keep their values
static int download_f(evpk_ctx *c, double *host, int f, int mode, const unsigned char *act = nullptr) {
    if (!host || !c->nblocks) return 0;
    const size_t n = (size_t)c->nblocks * c->nyb * c->nxb;
    dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
    bool hostmem = false;
    if (double *dst = (double *)mapped_alias(host, n * sizeof(double), &hostmem)) {
        LAUNCH_BLOCKS(k_scatter_f, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, f, dst, mode, act);
        HIPCHK(c, hipGetLastError());
        if (c->verify_delivery && hostmem) {
            HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->stage, (int)DV_SENTINEL32, 2 * n, c->stream));
            LAUNCH_BLOCKS(k_scatter_f, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, f, c->stage, mode, act);
            HIPCHK(c, hipGetLastError());
            return verify_plane(c, host, sizeof(double), n, f, "field");
        }
        return 0;
    }
    HIPCHK(c, hipMemcpyAsync(c->stage, host, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    LAUNCH_BLOCKS(k_scatter_f, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, f, c->stage, mode);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(host, c->stage, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the staging buffer is reused by the next field
    return 0;
}

static int download_m(evpk_ctx *c, int32_t *host, const int32_t *dev_plane, int mode) {
    if (!host || !c->nblocks) return 0;
    const size_t n = (size_t)c->nblocks * c->nyb * c->nxb;
    dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
    bool hostmem = false;
    if (int32_t *dst = (int32_t *)mapped_alias(host, n * sizeof(int32_t), &hostmem)) {
        LAUNCH_BLOCKS(k_scatter_m, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, dev_plane, dst, mode);
        HIPCHK(c, hipGetLastError());
        if (c->verify_delivery && hostmem) {
            HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->stage, (int)DV_SENTINEL32, n, c->stream));
            LAUNCH_BLOCKS(k_scatter_m, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, dev_plane, (int32_t *)c->stage, mode);
            HIPCHK(c, hipGetLastError());
            return verify_plane(c, host, sizeof(int32_t), n, -1, "mask");
        }
        return 0;
    }
    HIPCHK(c, hipMemcpyAsync(c->stage, host, n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    LAUNCH_BLOCKS(k_scatter_m, g, b, 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, dev_plane, (int32_t *)c->stage, mode);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(host, c->stage, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- transport primitives (device pointers, ordered on the stream given) -----------------------------------
static inline int xp_channel(const evpk_ctx *c, hipStream_t st) { return (st && st == c->stream2) ? 1 : 0; }

// peer-mapped transport: buffers of the NEXT message to / from a rank on a channel (half `part` of the slot), then the
// signal / wait that turn the page
static double *ipc_send_ptr(evpk_ctx *c, int ch, int dst, int part) {
    IpcXp &x = *c->ipc;
    return reinterpret_cast<double *>(x.peer[dst] + x.slot_off(ch, (x.sent[ch][dst] + 1) & 1, x.rank) + (size_t)part * (x.slot[ch] / 2));
}
static double *ipc_recv_ptr(evpk_ctx *c, int ch, int src, int part) {
    IpcXp &x = *c->ipc;
    return reinterpret_cast<double *>(x.mybox + x.slot_off(ch, (x.recvd[ch][src] + 1) & 1, src) + (size_t)part * (x.slot[ch] / 2));
}
static int ipc_signal(evpk_ctx *c, int ch, int dst, hipStream_t st) {
    IpcXp &x = *c->ipc;
    hipLaunchKernelGGL(k_ipc_signal, dim3(1), dim3(1), 0, st, x.flag(ch, x.rank, dst), (unsigned)++x.sent[ch][dst]);
    HIPCHK(c, hipGetLastError());
    return 0;
}
static int ipc_wait(evpk_ctx *c, int ch, int src, hipStream_t st) {
    IpcXp &x = *c->ipc;
    hipLaunchKernelGGL(k_ipc_wait, dim3(1), dim3(1), 0, st, (const unsigned *)x.flag(ch, src, x.rank), (unsigned)++x.recvd[ch][src], x.d_err,
                       2000000000ull /* 20 s of the 100 MHz clock */);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// Ring exchange with the west / east neighbour in two steps, so that a transport with mapped buffers can hand out the
// NEIGHBOUR'S memory as the place to pack into.  xp_ring_bufs: where the pack kernel puts the message for the west (sW) and
// east (sE) neighbour and where the unpack kernel will find the messages from the east (rE) and west (rW) neighbour;
// lsend / lrecv: local buffers [to west | to east] / [from east | from west] for the transports that move the bytes
// themselves.  xp_ring: deliver (counts in doubles).  With two ranks on a cyclic ring the neighbours coincide and one
// message [sW | sE] goes each way, received as [rE | rW].
struct RingBufs { double *sW, *sE, *rE, *rW; };
static void xp_ring_bufs(evpk_ctx *c, hipStream_t st, double *lsend, size_t nSW, double *lrecv, size_t nRE, RingBufs *b) {
    b->sW = lsend; b->sE = lsend + nSW; b->rE = lrecv; b->rW = lrecv + nRE;
    if (c->ipc) {
        const int ch = xp_channel(c, st);
        if (c->west >= 0) { b->sW = ipc_send_ptr(c, ch, c->west, 0); b->rW = ipc_recv_ptr(c, ch, c->west, 1); }
        if (c->east >= 0) { b->sE = ipc_send_ptr(c, ch, c->east, 1); b->rE = ipc_recv_ptr(c, ch, c->east, 0); }
    }
}
// phase: XP_ALL, or XP_POST (the peer-mapped transport rings the neighbours; the others do nothing yet) followed later by XP_DONE (it
// waits for them; RCCL / the relay move the bytes) -- so that another exchange can be posted in between (zone_mirror_exchange)
enum { XP_ALL = 0, XP_POST = 1, XP_DONE = 2 };
static int xp_ring(evpk_ctx *c, const RingBufs &b, size_t nSW, size_t nSE, size_t nRE, size_t nRW, hipStream_t st = nullptr, int phase = XP_ALL) {
    if (!st) st = c->stream;
    const bool merged = (c->west == c->east && c->west >= 0);
    if (c->ipc) {
        const int ch = xp_channel(c, st);
        if (phase != XP_DONE) {
            if ((nSW > c->ipc->slot[ch] / 16) || (nSE > c->ipc->slot[ch] / 16)) FAIL(c, "ipc transport: message larger than its slot");
            if (c->west >= 0 && ipc_signal(c, ch, c->west, st)) return 1;
            if (c->east >= 0 && !merged && ipc_signal(c, ch, c->east, st)) return 1;
        }
        if (phase != XP_POST) {
            if (c->east >= 0 && ipc_wait(c, ch, c->east, st)) return 1;
            if (c->west >= 0 && !merged && ipc_wait(c, ch, c->west, st)) return 1;
        }
        return 0;
    }
    if (phase == XP_POST) return 0;
    if (merged && (b.sE != b.sW + nSW || b.rW != b.rE + nRE)) FAIL(c, "xp_ring: merged message needs contiguous buffers");
    if (c->relay) {
        int rc = 0;
        if (merged) {
            rc |= c->relay->send(c->west, b.sW, (nSW + nSE) * 8, st);
            rc |= c->relay->recv(c->west, b.rE, (nRE + nRW) * 8, st);
        } else {
            if (c->west >= 0) rc |= c->relay->send(c->west, b.sW, nSW * 8, st);
            if (c->east >= 0) rc |= c->relay->send(c->east, b.sE, nSE * 8, st);
            if (c->east >= 0) rc |= c->relay->recv(c->east, b.rE, nRE * 8, st);
            if (c->west >= 0) rc |= c->relay->recv(c->west, b.rW, nRW * 8, st);
        }
        if (rc) FAIL(c, "shared-memory relay: exchange failed (%s)", rc & 2 ? "timeout" : "copy / size");
        return 0;
    }
    // (a failing call must not leave the thread inside an open group: every later RCCL call, ncclCommDestroy included,
    // would be queued and never issued -- collect the codes, always close the group, then report)
    NCCLCHK(c, ncclGroupStart());
    ncclResult_t rc = ncclSuccess;
    auto keep = [&](ncclResult_t e) { if (rc == ncclSuccess) rc = e; };
    if (merged) {
        if (nSW + nSE) keep(ncclSend(b.sW, nSW + nSE, ncclDouble, c->west, c->comm, st));
        if (nRE + nRW) keep(ncclRecv(b.rE, nRE + nRW, ncclDouble, c->west, c->comm, st));
    } else {
        if (c->west >= 0 && nSW) keep(ncclSend(b.sW, nSW, ncclDouble, c->west, c->comm, st));
        if (c->east >= 0 && nSE) keep(ncclSend(b.sE, nSE, ncclDouble, c->east, c->comm, st));
        if (c->east >= 0 && nRE) keep(ncclRecv(b.rE, nRE, ncclDouble, c->east, c->comm, st));
        if (c->west >= 0 && nRW) keep(ncclRecv(b.rW, nRW, ncclDouble, c->west, c->comm, st));
    }
    const ncclResult_t rce = ncclGroupEnd();
    if (rc != ncclSuccess) FAIL(c, "ncclSend/ncclRecv failed: %s", ncclGetErrorString(rc));
    if (rce != ncclSuccess) FAIL(c, "ncclGroupEnd failed: %s", ncclGetErrorString(rce));
    return 0;
}

// The tripole fold between x-slab ranks: every rank's two top rows of `nf` planes go to its fold partners (the mirror rank
// and the neighbours of it that hold the one or two columns beyond, mpi/ice_boundary.F90:2737-2913) and to itself; what
// arrives is scattered into the global-row buffer c->foldbuf.  One packed message per partner and direction.
static int fold_p2p(evpk_ctx *c, int fp, int nf, int fprev, hipStream_t st) {
    Slab &s = c->s;
    const int tx = 128, ch = xp_channel(c, st);
    const size_t nseg = (size_t)nf * 2 * s.nxl, segcap = (size_t)c->max_nf * 2 * c->wmax;
    DstList dl{};
    SrcList sl{};
    dl.p[dl.n++] = c->foldseg;
    sl.p[sl.n] = c->foldseg; sl.i0[sl.n] = s.i0; sl.w[sl.n++] = s.nxl;
    if (c->ipc) {
        if (nseg * 8 > c->ipc->slot[ch] / 2) FAIL(c, "ipc transport: fold message larger than its slot");
        for (int q : c->fold_dst) dl.p[dl.n++] = ipc_send_ptr(c, ch, q, 0);
        for (int q : c->fold_src) { sl.p[sl.n] = ipc_recv_ptr(c, ch, q, 0); sl.i0[sl.n] = c->slab_i0[q]; sl.w[sl.n++] = c->slab_i0[q + 1] - c->slab_i0[q]; }
    } else {
        size_t k = 0;
        for (int q : c->fold_src) { sl.p[sl.n] = c->foldrcv + (k++) * segcap; sl.i0[sl.n] = c->slab_i0[q]; sl.w[sl.n++] = c->slab_i0[q + 1] - c->slab_i0[q]; }
    }
    hipLaunchKernelGGL(k_fold_pack_multi, dim3((s.nxl + tx - 1) / tx), dim3(tx), 0, st, s, fp, nf, dl, fprev);
    HIPCHK(c, hipGetLastError());
    if (c->ipc) {
        for (int q : c->fold_dst) if (ipc_signal(c, ch, q, st)) return 1;
        for (int q : c->fold_src) if (ipc_wait(c, ch, q, st)) return 1;
    } else if (c->relay) {
        int rc = 0;
        for (int q : c->fold_dst) rc |= c->relay->send(q, c->foldseg, nseg * 8, st);
        size_t k = 0;
        for (int q : c->fold_src) rc |= c->relay->recv(q, c->foldrcv + (k++) * segcap, (size_t)nf * 2 * (c->slab_i0[q + 1] - c->slab_i0[q]) * 8, st);
        if (rc) FAIL(c, "shared-memory relay: fold exchange failed");
    } else {
        NCCLCHK(c, ncclGroupStart());
        ncclResult_t rc = ncclSuccess;
        auto keep = [&](ncclResult_t e) { if (rc == ncclSuccess) rc = e; };
        for (int q : c->fold_dst) keep(ncclSend(c->foldseg, nseg, ncclDouble, q, c->comm, st));
        size_t k = 0;
        for (int q : c->fold_src) keep(ncclRecv(c->foldrcv + (k++) * segcap, (size_t)nf * 2 * (c->slab_i0[q + 1] - c->slab_i0[q]), ncclDouble, q, c->comm, st));
        const ncclResult_t rce = ncclGroupEnd();
        if (rc != ncclSuccess) FAIL(c, "fold exchange: ncclSend/ncclRecv failed: %s", ncclGetErrorString(rc));
        if (rce != ncclSuccess) FAIL(c, "fold exchange: ncclGroupEnd failed: %s", ncclGetErrorString(rce));
    }
    hipLaunchKernelGGL(k_fold_unpack, dim3((c->wmax + tx - 1) / tx, sl.n), dim3(tx), 0, st, nf, s.nxg, sl, c->foldbuf);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// all-gather of `bytes` per rank (multiple of 4) into dst[rank*bytes ...]
static int xp_allgather(evpk_ctx *c, const void *src, void *dst, size_t bytes, hipStream_t st = nullptr) {
    if (!st) st = c->stream;
    if (c->relay) {
        int rc = 0;
        for (int r = 0; r < c->xranks; r++) if (r != c->rank) rc |= c->relay->send(r, src, bytes, st);      // (every rank of the host: start-up only)
        for (int r = 0; r < c->xranks; r++) if (r != c->rank) rc |= c->relay->recv(r, (char *)dst + (size_t)r * bytes, bytes, st);
        if (rc) FAIL(c, "shared-memory relay: all-gather failed");
        HIPCHK(c, hipMemcpyAsync((char *)dst + (size_t)c->rank * bytes, src, bytes, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    NCCLCHK(c, ncclAllGather(src, dst, bytes / 4, ncclInt32, c->comm, st));
    return 0;
}

// peer-mapped transport: did a wait kernel give up (a partner rank that died or fell more than 20 s behind)?  Call after a
// stream synchronisation.
static int xp_check(evpk_ctx *c) {
    if (!c->ipc || !c->ipc->d_err) return 0;
    unsigned e = 0;
    HIPCHK(c, hipMemcpy(&e, c->ipc->d_err, sizeof(e), hipMemcpyDeviceToHost));
    if (e >> 16) FAIL(c, "ipc transport: a partner rank was more than one message ahead %u time(s) -- the ranks posted different exchanges; the results of this call are invalid", e >> 16);
    if (e) FAIL(c, "ipc transport: %u wait(s) on a partner rank timed out; the results of this call are invalid", e);
    return 0;
}

// the mirror slab M of band_pair holds the mirror rank's top XB rows: nylM = max(4, 2 zM + 1) rows + its two ghost rows
constexpr int XB_PLANES = 13;                                       // pair planes of the widest message (static fields of evpk_prep)
constexpr int XB_ROWS_MAX = 2 * ((ZW_MAX - 1) / 2) + 1 + 2;         // nylM + 2 at the deepest zones

// ---- rows r0 .. r0+nr-1 of the pair planes L (+ the mask bytes) of MY columns to every rank whose mirror slab holds some of
// them, and from the owners of the columns of MY mirror slab M into its rows m0 .. (band_pair): one message per partner and
// direction over the context's transport (a rank's own share -- the middle rank of an odd count mirrors onto itself -- stays
// on the device) ----
static size_t xb_bytes(const XbList &L, const XbSeg &G, int nr, int mask) {
    return ((size_t)L.np * nr * G.tot * sizeof(double2) + (mask ? (size_t)nr * G.tot : 0) + 15) & ~(size_t)15;
}
struct XbXchg { std::vector<const double2 *> rcv; const double2 *self = nullptr; int ch = 0; };
// phase XP_ALL, or XP_POST (pack; peer-mapped: ring the partners) / XP_DONE (the bytes arrive) / XP_UNPACK with the same XbXchg;
// chan >= 0: the peer-mapped channel to use instead of the stream's own
enum { XP_UNPACK = 3 };
static int xband_swap(evpk_ctx *c, const XbList &L, int r0, int m0, int nr, int mask, hipStream_t st, int phase = XP_ALL, XbXchg *xx = nullptr,
                      int chan = -1) {
    Slab &s = c->s;
    XbXchg loc;
    XbXchg &X = xx ? *xx : loc;
    const int tx = 128;
    if (phase == XP_ALL || phase == XP_POST) X.ch = chan >= 0 ? chan : xp_channel(c, st);
    const int ch = X.ch;
    auto sndp = [&](size_t k, int q) { return (c->ipc && q != c->rank) ? reinterpret_cast<double2 *>(ipc_send_ptr(c, ch, q, 0))
                                                                        : reinterpret_cast<double2 *>((char *)c->xb_send + k * c->xb_cap); };
    auto rcvp = [&](size_t k, int q) { return q == c->rank ? static_cast<const double2 *>(nullptr)
                                              : c->ipc ? reinterpret_cast<const double2 *>(ipc_recv_ptr(c, ch, q, 0))
                                                       : reinterpret_cast<const double2 *>((char *)c->xb_recv + k * c->xb_cap); };
    if (phase == XP_ALL || phase == XP_POST) {
        for (size_t k = 0; k < c->xb_to.size(); k++) {
            const auto &P = c->xb_to[k];
            const size_t bytes = xb_bytes(L, P.seg, nr, mask);
            if (bytes > c->xb_cap) FAIL(c, "xband_swap: message larger than its buffer");
            if (c->relay && P.rank != c->rank && bytes > c->relay->slot) FAIL(c, "shared-memory relay: band rows message larger than its slot");
            if (c->ipc && P.rank != c->rank && bytes > c->ipc->slot[ch] / 2) FAIL(c, "ipc transport: band rows message larger than its slot");
            double2 *snd = sndp(k, P.rank);
            if (P.rank == c->rank) X.self = snd;
            const dim3 g((unsigned)((P.seg.tot + tx - 1) / tx), (unsigned)(L.np * nr + (mask ? nr : 0)));
            hipLaunchKernelGGL(k_xband_pack, g, dim3(tx), 0, st, s, L, P.seg, r0, nr, mask, snd);
        }
        HIPCHK(c, hipGetLastError());
        X.rcv.resize(c->xb_from.size());          // (peer-mapped: the page of the NEXT message, before the wait turns it)
        for (size_t k = 0; k < c->xb_from.size(); k++) X.rcv[k] = rcvp(k, c->xb_from[k].rank);
        if (c->ipc)
            for (const auto &P : c->xb_to) if (P.rank != c->rank && ipc_signal(c, ch, P.rank, st)) return 1;
    }
    if (phase == XP_ALL || phase == XP_DONE) {
        if (c->ipc) {
            for (const auto &P : c->xb_from) if (P.rank != c->rank && ipc_wait(c, ch, P.rank, st)) return 1;
        } else if (c->relay) {
            int rc = 0;
            for (size_t k = 0; k < c->xb_to.size(); k++)
                if (c->xb_to[k].rank != c->rank) rc |= c->relay->send(c->xb_to[k].rank, sndp(k, c->xb_to[k].rank), xb_bytes(L, c->xb_to[k].seg, nr, mask), st);
            for (size_t k = 0; k < c->xb_from.size(); k++)
                if (c->xb_from[k].rank != c->rank)
                    rc |= c->relay->recv(c->xb_from[k].rank, (char *)c->xb_recv + k * c->xb_cap, xb_bytes(L, c->xb_from[k].seg, nr, mask), st);
            if (rc) FAIL(c, "shared-memory relay: band rows exchange failed");
        } else {
            NCCLCHK(c, ncclGroupStart());
            ncclResult_t rc = ncclSuccess;
            auto keep = [&](ncclResult_t e) { if (rc == ncclSuccess) rc = e; };
            for (size_t k = 0; k < c->xb_to.size(); k++)
                if (c->xb_to[k].rank != c->rank) keep(ncclSend(sndp(k, c->xb_to[k].rank), xb_bytes(L, c->xb_to[k].seg, nr, mask), ncclChar, c->xb_to[k].rank, c->comm, st));
            for (size_t k = 0; k < c->xb_from.size(); k++)
                if (c->xb_from[k].rank != c->rank)
                    keep(ncclRecv((char *)c->xb_recv + k * c->xb_cap, xb_bytes(L, c->xb_from[k].seg, nr, mask), ncclChar, c->xb_from[k].rank, c->comm, st));
            const ncclResult_t rce = ncclGroupEnd();
            if (rc != ncclSuccess || rce != ncclSuccess) FAIL(c, "band rows exchange: ncclSend / ncclRecv failed");
        }
    }
    if (phase == XP_ALL || phase == XP_UNPACK) {
        for (size_t k = 0; k < c->xb_from.size(); k++) {
            const auto &P = c->xb_from[k];
            const double2 *rcv = P.rank == c->rank ? X.self : X.rcv[k];
            if (!rcv) FAIL(c, "xband_swap: no message for the rank's own share of its mirror slab");
            const dim3 g((unsigned)((P.seg.tot + tx - 1) / tx), (unsigned)(L.np * nr + (mask ? nr : 0)));
            hipLaunchKernelGGL(k_xband_unpack, g, dim3(tx), 0, st, c->m, L, P.seg, m0, nr, mask, rcv);
        }
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}
// the state (u, v and the twelve stresses) of buffer SB: every row of M, ghost rows included <- the mirror rank's rows N-nylM .. N+1
static int xband_state(evpk_ctx *c, int SB, hipStream_t st, int phase = XP_ALL, XbXchg *xx = nullptr, int chan = -1) {
    XbList L{};
    for (int q = 0; q < NSTATE / 2; q++) L.f[L.np++] = SB + 2 * q;
    return xband_swap(c, L, c->s.nyl - c->m.nyl, 0, c->m.nyl + 2, 0, st, phase, xx, chan);
}

// ---- halo update of nf consecutive planes starting at f ---------------------------------
// fsrc_fold >= 0: ice_HaloUpdate_stress variant (only the tripole north ghost row of the
// destination planes is written, from the top physical row of the source planes).
// skip_ew: the caller refreshes the E-W ghost columns itself right after (exchange_cols carries them, all rows)
// fprev: see k_fold_pack (velocity updates inside the subcycle loop: the state buffer the kernel read)
static int halo(evpk_ctx *c, int f, int nf, bool necorner, bool vector, double fill, int fsrc_fold = -1, hipStream_t st_in = nullptr,
                bool skip_ew = false, int fprev = -1, int ew_from = 0, int loc_x = -1 /* 2: E face, 3: N face (k_fold_apply) */) {
    Slab &s = c->s;
    hipStream_t st = st_in ? st_in : c->stream;       // every launch, copy and transport call of this update
    const int tx = 128;
    const int gcol = (s.nxl + 2 + tx - 1) / tx, grow = (s.nyl + 2 + tx - 1) / tx;
    const bool stress_mode = fsrc_fold >= 0;
    if (nf > c->max_nf) FAIL(c, "halo: nf=%d exceeds buffer", nf);
    if (c->ns == EVPK_BND_CYCLIC) FAIL(c, "ns_boundary_type cyclic is not supported");
    if (c->ns == EVPK_BND_TRIPOLE && c->nranks == 1 && !c->force_exchange && necorner && loc_x < 0 && !stress_mode && s.nyl >= 3) {
        // single rank: the whole update of an NE-corner field in one launch
        const int n = std::max(std::max(s.nxg / 2 + 1, s.nxl + 2), s.nyl);
        hipLaunchKernelGGL(k_halo_tripole_ne1, dim3((n + tx - 1) / tx, 2), dim3(tx), 0, st,
                           s, f, nf, c->ew == EVPK_BND_CYCLIC ? 1 : 0, fill, vector ? -1.0 : 1.0, fprev, ew_from);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    // N-S
    if (c->ns == EVPK_BND_TRIPOLE) {
        if (!stress_mode) hipLaunchKernelGGL(k_halo_ns_fill, dim3(gcol), dim3(tx), 0, st, s, f, nf, fill, 0);
        const int fp = stress_mode ? fsrc_fold : f;
        if (c->nranks == 1 && !c->force_exchange) {
            hipLaunchKernelGGL(k_fold_pack, dim3((s.nxl + tx - 1) / tx), dim3(tx), 0, st, s, fp, nf, c->foldbuf, s.i0 - 1, fprev);
        } else if (c->nranks > 1) {
            // x-slabs: packed send / recv with the mirror ranks only
            if (fold_p2p(c, fp, nf, fprev, st)) return 1;
        } else {
            // forced exchange on one rank (tests): own segment [nf][2][wmax] through the all-gather path, re-packed into [nf][2][nxg]
            HIPCHK(c, hipMemsetAsync(c->foldloc, 0, sizeof(double) * (size_t)c->max_nf * 2 * c->wmax, st));
            Slab t = s; t.nxg = c->wmax;   // local segment addressed with gofs = 0
            hipLaunchKernelGGL(k_fold_pack, dim3((s.nxl + tx - 1) / tx), dim3(tx), 0, st, t, fp, nf, c->foldloc, 0, fprev);
            const size_t seg = (size_t)c->max_nf * 2 * c->wmax;
            if (c->comm) {
                if (xp_allgather(c, c->foldloc, c->foldall, seg * sizeof(double), st)) return 1;
            } else
                HIPCHK(c, hipMemcpyAsync(c->foldall, c->foldloc, sizeof(double) * seg, hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(k_fold_repack, dim3((s.nxg + tx - 1) / tx), dim3(tx), 0, st, nf, c->max_nf, c->nranks, c->wmax, s.nxg,
                               (const int *)c->d_slab_i0, (const double *)c->foldall, c->foldbuf);
        }
        // (x-slab ranks fold their own columns; the ghost columns of the two rows come with the E-W exchange that follows)
        hipLaunchKernelGGL(k_fold_apply, dim3(gcol), dim3(tx), 0, st, s, f, nf, (const double *)c->foldbuf,
                           stress_mode ? 0 : (loc_x >= 0 ? loc_x : (necorner ? 1 : 0)), (vector && !stress_mode) ? -1.0 : 1.0,
                           (c->nranks > 1 && !stress_mode) ? 1 : 0);
        HIPCHK(c, hipGetLastError());
        if (stress_mode) return 0;
    } else {
        hipLaunchKernelGGL(k_halo_ns_fill, dim3(gcol), dim3(tx), 0, st, s, f, nf, fill, 1);
    }
    // E-W over all rows (ghost rows included, which carries the corners)
    if (skip_ew) {
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    if (c->nranks == 1 && !c->force_exchange) {
        hipLaunchKernelGGL(k_halo_ew_local, dim3(grow), dim3(tx), 0, st, s, f, nf, c->ew == EVPK_BND_CYCLIC ? 1 : 0, fill);
    } else {
        // edge columns over all rows: [my W edge | my E edge] out, [east ghost | west ghost] in.
        // The W edge goes to the west neighbour (it is their east ghost), the E edge to the east one.
        const size_t cnt = (size_t)nf * (s.nyl + 2);
        RingBufs rb;
        xp_ring_bufs(c, st, c->sendbuf, cnt, c->recvbuf, cnt, &rb);
        hipLaunchKernelGGL(k_ew_pack, dim3(grow), dim3(tx), 0, st, s, f, nf, rb.sW, rb.sE);
        if (c->nranks == 1 && !c->comm) {   // forced exchange with myself (cyclic): my W edge is my own east ghost
            if (c->west >= 0) {
                HIPCHK(c, hipMemcpyAsync(rb.rE, rb.sW, sizeof(double) * cnt, hipMemcpyDeviceToDevice, st));
                HIPCHK(c, hipMemcpyAsync(rb.rW, rb.sE, sizeof(double) * cnt, hipMemcpyDeviceToDevice, st));
            }
        } else {
            if (xp_ring(c, rb, cnt, cnt, cnt, cnt, st)) return 1;
        }
        hipLaunchKernelGGL(k_ew_unpack, dim3(grow), dim3(tx), 0, st, s, f, nf, (const double *)rb.rW,
                           (const double *)rb.rE, c->west >= 0 ? 1 : 0, c->east >= 0 ? 1 : 0, fill);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ---- the twelve ice_HaloUpdate_stress calls after the loop (tripole): one pack, one all-gather, one apply ----------
static int halo_stress12(evpk_ctx *c, int f0) {
    Slab &s = c->s;
    const int tx = 128, nf = 12;
    const int gcol = (s.nxl + 2 + tx - 1) / tx;
    if (nf > c->max_nf) FAIL(c, "halo_stress12: buffer too small");
    if (c->nranks == 1 && !c->force_exchange) {
        hipLaunchKernelGGL(k_fold_pack, dim3((s.nxl + tx - 1) / tx), dim3(tx), 0, c->stream, s, f0, nf, c->foldbuf, s.i0 - 1, -1);
    } else if (c->nranks > 1) {
        if (fold_p2p(c, f0, nf, -1, c->stream)) return 1;
    } else {
        HIPCHK(c, hipMemsetAsync(c->foldloc, 0, sizeof(double) * (size_t)c->max_nf * 2 * c->wmax, c->stream));
        Slab t = s; t.nxg = c->wmax;
        hipLaunchKernelGGL(k_fold_pack, dim3((s.nxl + tx - 1) / tx), dim3(tx), 0, c->stream, t, f0, nf, c->foldloc, 0, -1);
        const size_t seg = (size_t)c->max_nf * 2 * c->wmax;
        if (c->comm) {
            if (xp_allgather(c, c->foldloc, c->foldall, seg * sizeof(double))) return 1;
        } else
            HIPCHK(c, hipMemcpyAsync(c->foldall, c->foldloc, sizeof(double) * seg, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(k_fold_repack, dim3((s.nxg + tx - 1) / tx), dim3(tx), 0, c->stream, nf, c->max_nf, c->nranks, c->wmax, s.nxg,
                           (const int *)c->d_slab_i0, (const double *)c->foldall, c->foldbuf);
    }
    hipLaunchKernelGGL(k_fold_apply_stress12, dim3(gcol), dim3(tx), 0, c->stream, s, f0, (const double *)c->foldbuf);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ---- run-time flags -> template arguments ------------------------------------------------------------------
// with_bool(flag, f) calls f(std::true_type{}) or f(std::false_type{}): inside f, decltype(B)::value is a constant expression.
// Every kernel family below maps its flags to template arguments in ONE place; only combinations that are written out there are
// instantiated (evpk_kernels.hip instantiates exactly those explicitly).
template <class F> static inline void with_bool(bool flag, F &&f) {
    if (flag) f(std::true_type{}); else f(std::false_type{});
}
template <class F> static inline void with_bool(bool flag1, bool flag2, F &&f) {
    with_bool(flag1, [&](auto B1) { with_bool(flag2, [&](auto B2) { f(B1, B2); }); });
}
// the ridging and ITD kernels are built for five categories (<5>) and for any number (<0>): inside f, decltype(NC)::value is that argument
template <class F> static inline void with_ncat(int ncat, F &&f) {
    if (ncat == 5) f(std::integral_constant<int, 5>{}); else f(std::integral_constant<int, 0>{});
}
// the column kernels are built for five categories of four ice layers and one snow layer (<5, 4, 1>) and for any sizes (<0, 0, 0>)
template <class F> static inline void with_layers(int ncat, int nilyr, int nslyr, F &&f) {
    using std::integral_constant;
    if (ncat == 5 && nilyr == 4 && nslyr == 1) f(integral_constant<int, 5>{}, integral_constant<int, 4>{}, integral_constant<int, 1>{});
    else f(integral_constant<int, 0>{}, integral_constant<int, 0>{}, integral_constant<int, 0>{});
}

// a knob that is on unless the environment sets it to 0 (read per call)
static bool env_on(const char *name) { const char *v = getenv(name); return !(v && atoi(v) == 0); }
// one workgroup row per row of a caller's block array, one grid layer per local block (LAUNCH_BLOCKS)
static inline dim3 block_grid(const evpk_ctx *c) { return dim3((c->nxb + 63) / 64, c->nyb, c->nblocks); }
// a launch of that shape on c->stream: kernel(slab, block descriptors, args...)
template <class K, class... A> static int launch_blocks(evpk_ctx *c, K kernel, const A &...args) {
    hipLaunchKernelGGL(kernel, block_grid(c), dim3(64), 0, c->stream, c->s, (const BlockDesc *)c->d_bd, args...);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// workgroups of a launch (or of one part of it: strips, band, mirror slab) rounded up to a multiple of 8: XCD remap in the kernels
static inline int xcd_round(int nwg) { return (nwg + 7) & ~7; }

// ---- launch of the two-subcycle kernel (marching k_subcycle2p or one of the tile kernels) ------------------
static void launch_sub2(evpk_ctx *c, const SubArgs &a_in, hipStream_t st, bool revp, bool last2) {
    // The tripole band (and mirror-slab) workgroups as the LAST of the grid (round 5) -- in the marching kernel only.  There the
    // strips of a launch take (nearly) all workgroup slots for ~200 us and 30 band workgroups of ~50 us in FRONT of them pushed
    // the last strips into a second round: 0.2026 -> 0.1976 ms per launch, 12.85 -> 12.54 ms per evp at 3600x2700
    // (profiles/r05_v1/band_last_ab.txt).  A tile launch is SHORTER than a band workgroup's chain of four phases and two folds:
    // started last, the band is all that is left running (1440x1080 tripole 2.90 -> 3.40 ms per evp): there it stays first.
    SubArgs a = a_in;
    a.band_last = (c->band_last && !c->tile_mode) ? 1 : 0;
    const bool xm = a.nmir > 0 && !last2 && a.xm;      // ... then the strips of the mirror slab (x-slab ranks, XM kernels)
    // the strips (tile kernels: one per workgroup, marching kernels: four), then the tripole top band as workgroups of the pair's
    // own launch (band_pair), then the strips of the mirror slab
    const int per_wg = c->tile_mode ? 1 : 4;
    const dim3 g(xcd_round((a.nstrips + per_wg - 1) / per_wg) + xcd_round(a.nband) + (xm ? xcd_round((a.nmir + per_wg - 1) / per_wg) : 0));
    const size_t band_lds = a.nband ? sizeof(double) * BAND_LDS_DOUBLES : (size_t)0;
    // XM excludes LAST2 (the mirror slab is only advanced when another pair follows): <*, true, *, true> is never named
    with_bool(revp, [&](auto RV) {
        constexpr bool rv = decltype(RV)::value;
        if (c->tile_mode) {                      // small-slab variant: one workgroup of R + 3 waves per strip, one row per wave
            const dim3 b((a.R + 3) * 64);
            const size_t lds = std::max((size_t)(a.R + 3) * (4096 + 5 * 1024), band_lds);
            if (xm) hipLaunchKernelGGL((k_subcycle2t<rv, false, true>), g, b, lds, st, a);
            else if (last2 && a.R + 3 <= 8) hipLaunchKernelGGL(k_subcycle2t8<rv>, g, b, lds, st, a);      // (no scratch)
            else with_bool(last2, [&](auto L2) { hipLaunchKernelGGL((k_subcycle2t<rv, decltype(L2)::value>), g, b, lds, st, a); });
        } else {                                 // marching, the next row prefetched through LDS
            const dim3 b(256);
            if (xm) with_bool(c->compact, [&](auto CMX) { hipLaunchKernelGGL((k_subcycle2p<rv, false, decltype(CMX)::value, true>), g, b, 0, st, a); });
            else with_bool(last2, c->compact, [&](auto L2, auto CMX) { hipLaunchKernelGGL((k_subcycle2p<rv, decltype(L2)::value, decltype(CMX)::value>), g, b, 0, st, a); });
        }
    });
}

// one subcycle, one row per wave (k_subcycle_t): the band launches of a tripole pair -- their sequence is on the critical path of
// every pair -- and the one-subcycle launch of a small slab
static void launch_sub1t(const SubArgs &a, hipStream_t st, bool revp, bool last) {
    with_bool(last, revp, [&](auto LAST, auto RV) {
        hipLaunchKernelGGL((k_subcycle_t<decltype(LAST)::value, decltype(RV)::value>), dim3(a.nstrips), dim3((a.R + 1) * 64), (size_t)(a.R + 1) * 2048, st, a);
    });
}

// one subcycle, marching: four strips per workgroup (k_subcycle)
static void launch_sub1(const SubArgs &a, hipStream_t st, bool revp, bool last) {
    with_bool(last, revp, [&](auto LAST, auto RV) {
        hipLaunchKernelGGL((k_subcycle<decltype(LAST)::value, decltype(RV)::value>), dim3(xcd_round((a.nstrips + 3) / 4)), dim3(256), 0, st, a);
    });
}

// ---- ghost zones (zW columns per side) of a list of pair planes: x-slab neighbours ------------------------
// compact: only the rows of the four zone windows that hold an active cell (lists made at prep), else all rows
struct ColsXchg { RingBufs rb; ZoneRows zr; size_t nSW, nSE, nRE, nRW; int npr; };
static int exchange_cols(evpk_ctx *c, const PairList &pl, bool compact, int phase = XP_ALL, ColsXchg *cx = nullptr) {
    Slab &s = c->s;
    ColsXchg loc;
    ColsXchg &Q = cx ? *cx : loc;
    if (phase == XP_DONE) return xp_ring(c, Q.rb, 2 * Q.nSW, 2 * Q.nSE, 2 * Q.nRE, 2 * Q.nRW, nullptr, XP_DONE);
    if (phase == XP_UNPACK) {
        if (Q.npr > 0) hipLaunchKernelGGL(k_cols_unpack, dim3((Q.npr + 255) / 256), dim3(256), 0, c->stream, s, pl, c->zW, Q.zr, (const double2 *)Q.rb.rW,
                                          (const double2 *)Q.rb.rE, c->west >= 0 ? 1 : 0, c->east >= 0 ? 1 : 0);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    const int W = c->zW, rows = s.nyl + 2;
    const int npl = pl.n + (pl.with_cmask ? 1 : 0);
    if (npl > 25) FAIL(c, "exchange_cols: too many planes");
    ZoneRows zr;
    if (compact) {
        zr.sW = RowSet{c->d_zrows + 0 * rows, c->zn[0]}; zr.sE = RowSet{c->d_zrows + 1 * rows, c->zn[1]};
        zr.rE = RowSet{c->d_zrows + 2 * rows, c->zn[2]}; zr.rW = RowSet{c->d_zrows + 3 * rows, c->zn[3]};
    } else
        zr.sW = zr.sE = zr.rE = zr.rW = RowSet{nullptr, rows};
    // double2 elements per message; the slots are laid out back to back with the actual sizes (merged messages)
    const size_t nSW = (size_t)npl * zr.sW.n * W, nSE = (size_t)npl * zr.sE.n * W;
    const size_t nRE = (size_t)npl * zr.rE.n * W, nRW = (size_t)npl * zr.rW.n * W;
    RingBufs rb;      // (double2 elements counted in doubles for the transport)
    xp_ring_bufs(c, c->stream, (double *)c->cbuf, 2 * nSW, (double *)(c->cbuf + 2 * c->cslot), 2 * nRE, &rb);
    double2 *sendW = (double2 *)rb.sW, *sendE = (double2 *)rb.sE, *recvE = (double2 *)rb.rE, *recvW = (double2 *)rb.rW;
    const int tx = 256;
    const int nps = std::max(zr.sW.n, zr.sE.n) * W, npr = std::max(zr.rE.n, zr.rW.n) * W;
    if (nps > 0) hipLaunchKernelGGL(k_cols_pack, dim3((nps + tx - 1) / tx), dim3(tx), 0, c->stream, s, pl, W, zr, sendW, sendE);
    if (c->nranks == 1 && !c->comm) {   // forced exchange with myself (cyclic ring of one)
        if (c->west >= 0) {
            if (nSW != nRE || nSE != nRW) FAIL(c, "exchange_cols: self-exchange row sets differ");
            if (nSW) HIPCHK(c, hipMemcpyAsync(recvE, sendW, sizeof(double2) * nSW, hipMemcpyDeviceToDevice, c->stream));
            if (nSE) HIPCHK(c, hipMemcpyAsync(recvW, sendE, sizeof(double2) * nSE, hipMemcpyDeviceToDevice, c->stream));
        }
    } else {
        Q.rb = rb; Q.zr = zr; Q.nSW = nSW; Q.nSE = nSE; Q.nRE = nRE; Q.nRW = nRW; Q.npr = npr;
        if (xp_ring(c, rb, 2 * nSW, 2 * nSE, 2 * nRE, 2 * nRW, nullptr, phase)) return 1;
        if (phase == XP_POST) { HIPCHK(c, hipGetLastError()); return 0; }
    }
    if (npr > 0) hipLaunchKernelGGL(k_cols_unpack, dim3((npr + tx - 1) / tx), dim3(tx), 0, c->stream, s, pl, W, zr, (const double2 *)recvW,
                       (const double2 *)recvE, c->west >= 0 ? 1 : 0, c->east >= 0 ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    return 0;
}

static PairList state_pairs(int SB) {
    PairList pl{};
    for (int q = 0; q < NSTATE / 2; q++) pl.p[pl.n++] = (SB >> 1) + q;
    return pl;
}

static void destroy_impl(evpk_ctx *c) {
    if (!c) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->h_counts) { (void)hipHostFree(c->h_counts); c->h_counts = nullptr; }      // (after the async copies into it have drained)
    if (c->comm) (void)ncclCommDestroy(c->comm);
    if (c->relay) { c->relay->close_(); delete c->relay; }
    if (c->ipc) { if (c->stream2) (void)hipStreamSynchronize(c->stream2); c->ipc->close_(); delete c->ipc; }
    void *ptrs[] = {c->itd, c->stage_itd, c->d_zflags, c->d_zrows, c->s.F, c->s.tmask, c->s.umask, c->s.iceumask, c->s.cmask, c->s.tmphm, c->d_bd, c->stage, c->d_flags,
                    c->d_strips, c->d_counts, c->tile_buf, c->d_tune, c->d_flags2, c->d_strips2, c->d_strips2e, c->d_strips2i, c->d_band, c->cbuf, c->sendbuf, c->recvbuf, c->foldbuf, c->foldloc, c->foldall, c->d_slab_i0, c->foldseg, c->foldrcv, c->io_raw, c->io_act, c->tp_a, c->tp_b, c->call_stage, c->rm_grid, c->rm_pool, c->rm_tab, c->rm_sgn, c->rm_bad, c->uw_pool, c->uw_tab, c->uw_sgn, c->rg_pool, c->rg_mask, c->rg_flags, c->rg_ctl, c->itd_bmask, c->itd_key, c->th1_pool, c->dyn_stage, c->d_ns2, c->d_bmap, c->br_buf, c->m.F, c->m.cmask, c->d_mslab, c->xb_send, c->xb_recv, c->d_mstrips, c->eap_pool, c->eap_tab, c->sigB, c->sigB1, c->d_dbg, c->up_dat};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->evI) (void)hipEventDestroy(c->evI);
    if (c->evX) (void)hipEventDestroy(c->evX);
    if (c->evE) (void)hipEventDestroy(c->evE);
    if (c->evB0) (void)hipEventDestroy(c->evB0);
    if (c->evB1) (void)hipEventDestroy(c->evB1);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    for (auto e : c->kev) (void)hipEventDestroy(e);
    for (auto e : c->bev) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int evpk_destroy(evpk_ctx *c) { destroy_impl(c); return 0; }

// ---- second phase of the start: everything that involves the other ranks (collective) ----------------------------
static int connect_impl(evpk_ctx *c, const void *unique_id) {
    if (c->connected) FAIL(c, "evpk_connect: the context is connected already");
    Slab &s = c->s;
    const int i0 = s.i0, i1 = s.i0 + s.nxl - 1;
    hipDeviceProp_t prop;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
    if (c->xranks > 1) {
        if (!unique_id) FAIL(c, "nranks > 1 needs a unique id (evpk_get_unique_id on rank 0, broadcast by the host)");
        char nm[EVPK_UNIQUE_ID_BYTES + 1];
        memcpy(nm, (const char *)unique_id + 8, EVPK_UNIQUE_ID_BYTES - 8);
        nm[EVPK_UNIQUE_ID_BYTES - 8] = 0;
        if (strncmp((const char *)unique_id, "EVPKSHM:", 8) == 0) {
            // test transport: host-staged relay through POSIX shared memory (several ranks on one GPU)
            const size_t slot = std::max<size_t>((size_t)2 * c->cslot * sizeof(double2),
                                                 (size_t)c->max_nf * 2 * (size_t)s.nxg * sizeof(double)) + 4096 +
                                (c->ns == EVPK_BND_TRIPOLE      // the band rows of xband_swap: at most a mirror slab's columns, zones included
                                     ? (size_t)(XB_PLANES * XB_ROWS_MAX * sizeof(double2) + XB_ROWS_MAX) * ((size_t)c->w_bound + 2 * ZW_MAX) + 64 : 0);
            c->relay = new ShmRelay();
            std::string err;
            if (c->relay->open(nm, c->rank, c->xranks, slot, err)) FAIL(c, "%s", err.c_str());
        } else if (strncmp((const char *)unique_id, "EVPKIPC:", 8) == 0) {
            // peer-mapped transport: start-up data through the POSIX segment (stage 1: slab starts)
            c->ipc = new IpcXp();
            std::string err;
            if (c->ipc->open(nm, c->rank, c->xranks, err)) FAIL(c, "%s", err.c_str());
            c->ipc->info(c->rank)->i0 = i0;
            c->ipc->set_stage(1);
            if (!c->ipc->wait_stage(1, err)) FAIL(c, "%s", err.c_str());
        } else {
            ncclUniqueId u;
            memcpy(&u, unique_id, sizeof(u));
            NCCLCHK(c, ncclCommInitRank(&c->comm, c->xranks, u, c->rank));
        }
        // every rank learns all slab starts (the tripole fold partners follow from them)
        // (collective over ALL the host's ranks; an idle rank reports nx_global + 1, the start of nothing)
        c->slab_i0.resize(c->xranks + 1);
        if (c->ipc) {
            for (int r = 0; r < c->xranks; r++) c->slab_i0[r] = c->ipc->info(r)->i0;
        } else {
            int *d_i0 = nullptr, *d_all = nullptr;
            HIPCHK(c, hipMalloc(&d_i0, sizeof(int)));
            HIPCHK(c, hipMalloc(&d_all, sizeof(int) * c->xranks));
            HIPCHK(c, hipMemcpyAsync(d_i0, &i0, sizeof(int), hipMemcpyHostToDevice, c->stream));
            if (xp_allgather(c, d_i0, d_all, sizeof(int))) return 1;
            HIPCHK(c, hipMemcpyAsync(c->slab_i0.data(), d_all, sizeof(int) * c->xranks, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            (void)hipFree(d_i0); (void)hipFree(d_all);
        }
        for (int r = c->nranks; r < c->xranks; r++)
            if (c->slab_i0[r] != s.nxg + 1) FAIL(c, "rank %d should own no block column (%d of %d ranks do) but reports columns from %d", r, c->nranks, c->xranks, c->slab_i0[r]);
        c->slab_i0.resize(c->nranks + 1);
        c->slab_i0[c->nranks] = s.nxg + 1;
        if (c->idle) {
            // the start-up stages of the peer-mapped transport are waited for by every rank; this one exports and maps nothing
            if (c->ipc) {
                std::string err;
                c->ipc->set_stage(2);
                if (!c->ipc->wait_stage(2, err)) FAIL(c, "%s", err.c_str());
                c->ipc->set_stage(3);
                if (!c->ipc->wait_stage(3, err)) FAIL(c, "%s", err.c_str());
            }
            c->connected = true;
            return 0;
        }
        c->wmax = 0;
        for (int r = 0; r < c->nranks; r++) {
            if (c->slab_i0[r + 1] <= c->slab_i0[r]) FAIL(c, "slabs are not ordered west to east by rank");
            c->wmax = std::max(c->wmax, c->slab_i0[r + 1] - c->slab_i0[r]);
        }
        if (c->slab_i0[c->rank] != i0 || c->slab_i0[c->rank + 1] != i1 + 1) FAIL(c, "slabs do not tile the global x range");
        if (c->ns == EVPK_BND_TRIPOLE) {
            // fold partners: rank r reads the rows at the mirrored columns nx - g (NE corner) and nx - g + 1 (centre) for
            // g = i0-1 .. i1+1 (the stress fold also fills its ghost columns), i.e. columns nx - i1 - 1 .. nx - i0 + 2; the
            // relation is kept symmetric (every pair swaps segments), which also keeps double buffering safe
            std::vector<char> pr((size_t)c->nranks * c->nranks, 0);
            auto owner = [&](int g) { while (g < 1) g += s.nxg; while (g > s.nxg) g -= s.nxg; int r = 0; while (g >= c->slab_i0[r + 1]) r++; return r; };
            for (int r = 0; r < c->nranks; r++)
                for (int g = s.nxg - (c->slab_i0[r + 1] - 1) - 1; g <= s.nxg - c->slab_i0[r] + 2; g++) {
                    const int q = owner(g);
                    if (q != r) pr[(size_t)r * c->nranks + q] = pr[(size_t)q * c->nranks + r] = 1;
                }
            for (int q = 0; q < c->nranks; q++) if (pr[(size_t)c->rank * c->nranks + q]) { c->fold_dst.push_back(q); c->fold_src.push_back(q); }
            if (c->fold_dst.size() > 5) FAIL(c, "tripole fold: %d partner ranks (slab widths too uneven)", (int)c->fold_dst.size());
            HIPCHK(c, hipMalloc(&c->foldseg, sizeof(double) * (size_t)c->max_nf * 2 * c->wmax));
            HIPCHK(c, hipMalloc(&c->foldrcv, sizeof(double) * (size_t)c->max_nf * 2 * c->wmax * std::max<size_t>(1, c->fold_src.size())));
        }
        if (c->ipc) {
            // stage 2: receive buffers of identical layout on every rank -- per channel [2 parities][nranks sources][slot]
            IpcXp &x = *c->ipc;
            const size_t fold_msg = (size_t)c->max_nf * 2 * c->wmax * sizeof(double);
            // (tripole: the band rows of xband_swap -- up to 12 pair planes x 5 rows + the mask bytes of a slab's columns and zones)
            const size_t xb_msg = c->ns == EVPK_BND_TRIPOLE ? ((size_t)(XB_PLANES * XB_ROWS_MAX * sizeof(double2) + XB_ROWS_MAX) * ((size_t)c->wmax + 2 * ZW_MAX) + 64) & ~(size_t)15 : 0;
            x.slot[0] = 2 * std::max<size_t>(std::max<size_t>(c->cslot * sizeof(double2), fold_msg), xb_msg);
            x.slot[1] = 2 * std::max<size_t>(std::max<size_t>((size_t)c->max_nf * (s.nyl + 2) * sizeof(double), fold_msg), xb_msg);   // (zone_mirror_exchange)
            x.chan_off[0] = 0;
            x.chan_off[1] = 2 * (size_t)x.nranks * x.slot[0];
            x.box_bytes = x.chan_off[1] + 2 * (size_t)x.nranks * x.slot[1];
            std::string err;
            {   // The receive buffers are written by kernels of OTHER devices while this device holds lines of them in
                // its L2s: uncached (fine-grained) device memory keeps that coherent without relying on the kernel-boundary
                // invalidates (what RCCL does for its own peer buffers); EVPK_IPC_MEM=coarse takes plain hipMalloc memory.
                const char *e = getenv("EVPK_IPC_MEM");
                const bool coarse = e && strcmp(e, "coarse") == 0;
                void *p = nullptr;
                if (coarse) {
                    HIPCHK(c, hipMalloc(&p, x.box_bytes));
                } else if (hipExtMallocWithFlags(&p, x.box_bytes, hipDeviceMallocUncached) != hipSuccess &&
                           hipExtMallocWithFlags(&p, x.box_bytes, hipDeviceMallocFinegrained) != hipSuccess) {
                    // no silent fall-back to cached memory: peers would store into lines this device's L2s may hold
                    (void)hipGetLastError();
                    FAIL(c, "ipc transport: neither uncached nor fine-grained device memory for the receive buffers (%zu bytes); "
                            "EVPK_IPC_MEM=coarse takes plain hipMalloc memory and relies on the kernel-boundary invalidates", x.box_bytes);
                }
                x.mybox = (char *)p;
            }
            HIPCHK(c, hipMemset(x.mybox, 0, x.box_bytes));
            hipIpcMemHandle_t h;
            HIPCHK(c, hipIpcGetMemHandle(&h, x.mybox));
            memcpy(x.handle(c->rank), &h, sizeof(h));
            x.set_stage(2);
            if (!x.wait_stage(2, err)) FAIL(c, "%s", err.c_str());
            for (int q = 0; q < c->nranks; q++) {
                if (q == c->rank) { x.peer[q] = x.mybox; continue; }
                hipIpcMemHandle_t hq;
                memcpy(&hq, x.handle(q), sizeof(hq));
                void *pq = nullptr;
                HIPCHK(c, hipIpcOpenMemHandle(&pq, hq, hipIpcMemLazyEnablePeerAccess));
                x.peer[q] = (char *)pq;
            }
            HIPCHK(c, hipHostRegister(x.base + x.flags_off, x.flags_bytes, hipHostRegisterMapped | hipHostRegisterPortable));
            x.registered = true;
            HIPCHK(c, hipHostGetDevicePointer((void **)&x.dflags, x.base + x.flags_off, 0));
            HIPCHK(c, hipMalloc(&x.d_err, sizeof(unsigned)));
            HIPCHK(c, hipMemset(x.d_err, 0, sizeof(unsigned)));
            x.set_stage(3);         // everything mapped: from here on only kernels touch the shared pages
            if (!x.wait_stage(3, err)) FAIL(c, "%s", err.c_str());
        }
    } else {
        c->slab_i0 = {1, s.nxg + 1};
        c->wmax = s.nxg;
        if (c->force_exchange && c->ns == EVPK_BND_TRIPOLE) {
            HIPCHK(c, hipMalloc(&c->foldloc, sizeof(double) * (size_t)c->max_nf * 2 * c->wmax));
            HIPCHK(c, hipMalloc(&c->foldall, sizeof(double) * (size_t)c->max_nf * 2 * c->wmax));
            HIPCHK(c, hipMalloc(&c->d_slab_i0, sizeof(int) * 2));
            HIPCHK(c, hipMemcpy(c->d_slab_i0, c->slab_i0.data(), sizeof(int) * 2, hipMemcpyHostToDevice));
        }
    }

    {   // two subcycles per launch: single rank, no tripole fold between the subcycles (EVPK_DOUBLE=0 disables)
        const char *e = getenv("EVPK_DOUBLE");
        // (the choice must be the same on every rank: it decides which exchanges the ranks post)
        int minw = s.nxl;
        for (int r = 0; r < c->nranks; r++) minw = std::min(minw, c->slab_i0[r + 1] - c->slab_i0[r]);
        c->use_double = !(e && atoi(e) == 0) && minw >= 4;
        if (c->ns == EVPK_BND_TRIPOLE) {
            // the fold mixes mirrored columns between the two fused subcycles: only the rows next to the fold are affected,
            // they are redone by band launches (x-slabs: without the edge/interior overlap, the fold all-gathers in between)
            c->band_mode = c->use_double = c->use_double && s.nyl >= 8;
        }
        // ghost-zone depth: zM launches per exchange, zones of 2*zM columns; every slab must be able to supply them
        const char *zm = getenv("EVPK_ZONE_M");
        int m = zm ? atoi(zm) : ZW_MAX / 2;
        m = std::max(1, std::min(m, std::min(ZW_MAX / 2, minw / 2)));
        // tripole between ranks without a per-subcycle exchange: see band_pair (every rank decides alike).  The mirror slab M of
        // rank d is a VIRTUAL slab of d's width that starts at global column nx - i0_d - w_d + 2 (NE-corner image of d's local
        // column i = M's local column w_d - i); its columns, ghost zones included, come from whichever ranks own them (cyclic):
        // the mirror rank P-1-d alone when the slabs are equal and P is even, up to three ranks (or d itself) otherwise
        std::vector<std::vector<XbSeg>> xsrc, xdst;     // [q][d]: runs of q's columns / of M_d's columns, message q -> d
        {
            const char *xe = getenv("EVPK_XBAND");
            if (const char *e = getenv("EVPK_XB_FUSE")) c->xb_fuse = atoi(e) != 0;
            // the merged refresh over RCCL (one ncclGroupStart / End around the sends and receives of the ghost zones AND the mirror slab,
            // several messages per peer in one group) has never run between two devices (1-GPU boxes: the multi-rank tests use the
            // peer-mapped transport): until a multi-GPU pass of tests/test_multirank_gpu.py has covered it, RCCL ranks meet twice per
            // refresh as in round 3 unless EVPK_XB_MERGE=1 asks for the merged form
            if (c->comm && c->nranks > 1) c->xb_merge = false;
            if (const char *e = getenv("EVPK_XB_MERGE")) c->xb_merge = atoi(e) != 0;
            bool ok = c->band_mode && c->nranks > 1 && c->band_fused && !(xe && atoi(xe) == 0) &&
                      minw >= 2 * ZW_MAX && s.nyl >= XB_ROWS_MAX + 1;
            if (ok) {
                const int P = c->nranks, nx = s.nxg;
                xsrc.assign(P, std::vector<XbSeg>(P, XbSeg{}));
                xdst.assign(P, std::vector<XbSeg>(P, XbSeg{}));
                auto owner = [&](int g) { int r = 0; while (g >= c->slab_i0[r + 1]) r++; return r; };
                for (int d = 0; d < P && ok; d++) {
                    const int wd = c->slab_i0[d + 1] - c->slab_i0[d], m0 = nx - c->slab_i0[d] - wd + 2;
                    if (wd + 2 * ZW_MAX > nx) { ok = false; break; }      // (a column would appear twice in M)
                    int lastq = -1, lastc = 0;
                    for (int cm = 1 - ZW_MAX; cm <= wd + ZW_MAX; cm++) {
                        int g = (m0 + cm - 2) % nx; if (g < 0) g += nx; g += 1;
                        const int q = owner(g), cq = g - c->slab_i0[q] + 1;
                        XbSeg &A = xsrc[q][d], &B = xdst[q][d];
                        if (q == lastq && cq == lastc + 1) { A.len[A.n - 1]++; B.len[B.n - 1]++; }
                        else if (A.n == 4) { ok = false; break; }
                        else { A.c0[A.n] = cq; A.len[A.n++] = 1; B.c0[B.n] = cm; B.len[B.n++] = 1; }
                        A.tot++; B.tot++;
                        lastq = q; lastc = cq;
                    }
                }
                // the exchange relation is symmetric (mirror of [i0 - Z, i0 + w - 1 + Z] under g -> nx - g + 1): the peer-mapped
                // transport's double buffering counts on every pair swapping messages
                for (int q = 0; q < P && ok; q++) for (int d = 0; d < P; d++) if ((xsrc[q][d].n != 0) != (xsrc[d][q].n != 0)) ok = false;
            }
            c->xband = ok;
        }
        if (c->band_mode && !c->xband) m = 1;          // the fold is exchanged after every subcycle anyway
        c->zM = m; c->zW = 2 * m;
        if (c->xband) {
            // the NE-corner fold maps my U column c to the partner's column w - c: the image of the zone [1-zW, w+zW] is
            // [-zW, w+zW-1], one column short of the partner's zone on its west side, so the band rows lose ONE more column
            // of validity on the east side than the rows below them (U valid up to w+zW-2k-1 after k pairs instead of
            // w+zW-2k) -- zones of 2m+1 columns pay for it
            m = std::min(m, (ZW_MAX - 1) / 2);
            c->zM = m; c->zW = 2 * m + 1;
            for (int q = 0; q < c->nranks; q++) {
                if (xsrc[c->rank][q].n) c->xb_to.push_back({q, xsrc[c->rank][q]});
                if (xdst[q][c->rank].n) c->xb_from.push_back({q, xdst[q][c->rank]});
            }
            c->m = s;
            // rows 1 .. nylM <-> rows N-nylM+1 .. N of the columns' owners, rows 0 and nylM+1 the row below / the north ghost row.
            // band_pair needs rows N-3 .. N+1; the rows below them are the ghost zone of the mirror slab IN Y: between two refreshes
            // M is advanced here like a slab of its own (the pair kernel over its strips), every pair of subcycles costing two rows
            // of validity from the bottom, so that one message per zM pairs -- sent together with the ghost-zone exchange --
            // replaces the message per pair that the four-row M of the first version needed
            c->m.nyl = std::max(4, 2 * m + 1);
            c->m.i0 = s.nxg - s.i0 - s.nxl + 2;
            c->m.tmask = c->m.umask = c->m.iceumask = nullptr;
            c->m.tmphm = c->m.tile_ice = c->m.tile_dat = c->m.act_ice = c->m.act_any = nullptr;
            HIPCHK(c, hipMalloc(&c->m.F, sizeof(double) * slab_doubles(c->m)));
            HIPCHK(c, hipMemset(c->m.F, 0, sizeof(double) * slab_doubles(c->m)));
            HIPCHK(c, hipMalloc(&c->m.cmask, mask_elems(c->m)));
            HIPCHK(c, hipMemset(c->m.cmask, 0, mask_elems(c->m)));
            HIPCHK(c, hipMalloc(&c->d_mslab, sizeof(Slab)));
            HIPCHK(c, hipMemcpy(c->d_mslab, &c->m, sizeof(Slab), hipMemcpyHostToDevice));
            // one buffer per partner and direction, each large enough for the widest message (the static fields of evpk_prep)
            size_t cols = 0;
            for (const auto &P : c->xb_to) cols = std::max(cols, (size_t)P.seg.tot);
            for (const auto &P : c->xb_from) cols = std::max(cols, (size_t)P.seg.tot);
            c->xb_cap = ((size_t)XB_PLANES * (c->m.nyl + 2) * cols * sizeof(double2) + (size_t)(c->m.nyl + 2) * cols + 64) & ~(size_t)15;
            HIPCHK(c, hipMalloc(&c->xb_send, c->xb_cap * c->xb_to.size()));
            HIPCHK(c, hipMalloc(&c->xb_recv, c->xb_cap * c->xb_from.size()));
        }
        std::vector<int> band(c->ncx);
        for (int k = 0; k < c->ncx; k++) band[k] = k;
        HIPCHK(c, hipMalloc(&c->d_band, sizeof(int) * c->ncx));
        HIPCHK(c, hipMemcpy(c->d_band, band.data(), sizeof(int) * c->ncx, hipMemcpyHostToDevice));
    }
    {   // resident workgroups of the two-subcycle kernel variant this context launches (strip-height tuner)
        int nb = 0;
        const void *fn = c->compact ? (const void *)k_subcycle2p<false, false, true> : (const void *)k_subcycle2p<false, false, false>;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, 256, 0) == hipSuccess && nb > 0)
            c->slots2 = nb * prop.multiProcessorCount;
    }
    c->connected = true;
    return 0;
}

extern "C" int evpk_connect(evpk_ctx *c, const void *unique_id) {
    if (!c) return 1;
    return connect_impl(c, unique_id);
}

extern "C" int evpk_device_check(int32_t device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); g_create_err = "no HIP device: libevpk has no CPU fallback"; return 1; }
    if (device < 0 || device >= ndev) { g_create_err = "device " + std::to_string(device) + " out of range (" + std::to_string(ndev) + " devices)"; return 1; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void)hipGetLastError(); g_create_err = "hipGetDeviceProperties failed"; return 1; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { g_create_err = std::string("device is ") + prop.gcnArchName + ", libevpk is built for gfx950 only"; return 1; }
    return 0;
}

static int create_impl(evpk_ctx *c, const evpk_geom *g) {
    if (!g) FAIL(c, "geom is NULL");
    if (g->nblocks < 0 || g->nx_block < 3 || g->ny_block < 3) FAIL(c, "bad block shape");
    if (g->nranks < 1 || g->rank < 0 || g->rank >= g->nranks) FAIL(c, "bad rank/nranks");
    if (g->ns_boundary == EVPK_BND_CYCLIC) FAIL(c, "ns_boundary_type cyclic is not supported");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) FAIL(c, "no HIP device: libevpk has no CPU fallback");
    if (g->device < 0 || g->device >= ndev) FAIL(c, "device %d out of range (%d devices)", g->device, ndev);
    HIPCHK(c, hipSetDevice(g->device));
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, g->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) FAIL(c, "device is %s, libevpk is built for gfx950 only", prop.gcnArchName);
    c->device = g->device;
    c->nxb = g->nx_block; c->nyb = g->ny_block; c->nblocks = g->nblocks;
    c->ew = g->ew_boundary; c->ns = g->ns_boundary; c->rank = g->rank; c->xranks = g->nranks;
    {   // the ring of ranks that own block columns (every rank computes the same from the geometry)
        const int bsx = g->nx_block - 2, nbx = (g->nx_global - 1) / bsx + 1, nbx_pp = (nbx - 1) / g->nranks + 1;
        c->nranks = (nbx + nbx_pp - 1) / nbx_pp;
        if (g->rank >= c->nranks) {
            // no block column for this rank (e.g. 5 block columns on 4 ranks: 2, 2, 1, 0): it only takes part in evpk_connect
            if (g->nblocks != 0) FAIL(c, "rank %d owns no block column (%d block columns on %d ranks) but was given %d blocks", g->rank, nbx, g->nranks, g->nblocks);
            c->idle = true;
            c->s.nxg = g->nx_global; c->s.nyg = g->ny_global; c->s.i0 = g->nx_global + 1; c->s.nxl = 0;
            c->s.nyl = g->ny_global; c->s.j0 = 1;
            c->cslot = (size_t)25 * ZW_MAX * (c->s.nyl + 2);            // (the relay's mailboxes are sized alike on every rank)
            c->w_bound = std::min(nbx_pp * bsx, (int)g->nx_global);
            HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
            if (g->unique_id) return connect_impl(c, g->unique_id);
            return 0;
        }
    }

    // slab = bounding rectangle of the local blocks
    int i0 = 1 << 30, i1 = -1, j0 = 1 << 30, j1 = -1;
    long long covered = 0;
    c->bd.resize(g->nblocks);
    for (int b = 0; b < g->nblocks; b++) {
        BlockDesc d{g->ilo[b], g->ihi[b], g->jlo[b], g->jhi[b], g->iglob_lo[b], g->jglob_lo[b]};
        if (d.ilo < 2 || d.ihi > g->nx_block - 1 || d.ihi < d.ilo || d.jlo < 2 || d.jhi > g->ny_block - 1 || d.jhi < d.jlo)
            FAIL(c, "block %d: bad ilo/ihi/jlo/jhi", b);
        if (d.iglob_lo < 1 || d.jglob_lo < 1) FAIL(c, "block %d: bad global origin", b);
        // The fold rewrites the top physical row; the reference fills the ghost row of the block BELOW from its value before
        // that (regular copies first, tripole buffer second, ice_boundary.F90), so with a one-row top block the results
        // of the reference depend on the decomposition.  Not reproduced here.
        if (g->ns_boundary == EVPK_BND_TRIPOLE && d.jglob_lo + (d.jhi - d.jlo) == g->ny_global && d.jhi == d.jlo && g->ny_global > 1 &&
            d.jglob_lo > 1)
            FAIL(c, "tripole: the top row of blocks must hold at least two physical rows (block %d has one)", b);
        c->bd[b] = d;
        i0 = std::min(i0, d.iglob_lo); i1 = std::max(i1, d.iglob_lo + d.ihi - d.ilo);
        j0 = std::min(j0, d.jglob_lo); j1 = std::max(j1, d.jglob_lo + d.jhi - d.jlo);
        covered += (long long)(d.ihi - d.ilo + 1) * (d.jhi - d.jlo + 1);
    }
    if (i1 > g->nx_global || j1 > g->ny_global) FAIL(c, "blocks exceed the global grid");
    // The slab is the rank's share of the DOMAIN, not the bounding box of the blocks that survived land-block elimination
    // (ice_domain.F90:387-441: blocks without ocean are dropped, e.g. the all-land southern rows of a global grid): the
    // x range follows create_distrb_cart's arithmetic for slenderX1 (ice_distribution.F90:603-640: contiguous ranges of
    // ceil(nblocks_x / nprocs) block columns), the y range is the whole grid.  Cells no block covers read as land.
    {
        const int bsx = g->nx_block - 2, nbx = (g->nx_global - 1) / bsx + 1, nbx_pp = (nbx - 1) / g->nranks + 1;
        const int r0 = g->rank * nbx_pp * bsx + 1, r1 = std::min((g->rank + 1) * nbx_pp * bsx, (int)g->nx_global);
        if (i0 < r0 || i1 > r1)
            FAIL(c, "%s (blocks span i %d..%d, the rank's share is %d..%d)", g->nranks > 1 ? "multi-rank runs need x-slabs of whole columns (processor_shape slenderX1)"
                                                                                        : "single-rank context: blocks outside the grid", i0, i1, r0, r1);
        i0 = r0; i1 = r1; j0 = 1; j1 = g->ny_global;
        c->w_bound = std::min(nbx_pp * bsx, (int)g->nx_global);          // no rank's slab is wider (every rank computes the same)
    }
    Slab &s = c->s;
    s.nxl = i1 - i0 + 1; s.nyl = j1 - j0 + 1; s.i0 = i0; s.j0 = j0; s.nxg = g->nx_global; s.nyg = g->ny_global;
    if (g->ns_boundary == EVPK_BND_TRIPOLE && (s.nyl < 2 || (g->nx_global & 1))) FAIL(c, "tripole needs ny >= 2 and even nx_global");
    // (with 'open' / 'closed' E-W the reference's copy out of the tripole buffer follows mirrored ghost indices resp. reads
    //  column nx_global + 1 of the buffer in ice_HaloUpdate_stress: serial/ice_boundary.F90:3752-3776, :3420-3424)
    if (g->ns_boundary == EVPK_BND_TRIPOLE && g->ew_boundary != EVPK_BND_CYCLIC) FAIL(c, "a tripole grid must be cyclic in the E-W direction");
    c->full_cover = (covered == (long long)s.nxl * s.nyl);
    s.pitch = ((C0 + s.nxl + ZW_MAX + 1 + 7) / 8) * 8;     // columns 1-ZW_MAX .. nxl+ZW_MAX (ghost zones of up to ZW_MAX columns per side)
    s.rstride = NP * s.pitch;

    {   // `stream` carries the edge strips and the neighbour exchange (pack, RCCL, unpack): dispatched ahead of the
        // interior strips on `stream2`, which only have to be done by the next launch
        int least = 0, greatest = 0;
        HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(c, hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, greatest));
        // (tripole: stream2 carries the band launches and folds beside the main launch -- few, short, urgent)
        HIPCHK(c, hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking,
                                              (c->nranks > 1 && g->ns_boundary != EVPK_BND_TRIPOLE) ? least : greatest));
    }
    {   // hand-over events between the two streams of THIS device: a device-scope release is all they need (the system-scope
        // fence of a default event costs ~4 us per hand-over; EVPK_EVENT_SCOPE=0 restores it)
        unsigned fl = hipEventDisableTiming | hipEventReleaseToDevice;
        const char *e = getenv("EVPK_EVENT_SCOPE");
        if (e && atoi(e) == 0) fl = hipEventDisableTiming;
        HIPCHK(c, hipEventCreateWithFlags(&c->evB0, fl));
        HIPCHK(c, hipEventCreateWithFlags(&c->evB1, fl));
        {
            const char *hv = getenv("EVPK_HANDOVER");
            int can = 0;
            (void)hipDeviceGetAttribute(&can, hipDeviceAttributeCanUseStreamWaitValue, c->device);
            // (one rank only: with several rank processes on ONE device -- the functional multi-rank checks -- queues blocked in a
            // value wait and the partner ranks' spinning exchange kernels starve each other; between ranks the events stay)
            if (hv && !strcmp(hv, "value") && can && c->nranks == 1) {
                if (hipExtMallocWithFlags((void **)&c->sigB, 8, hipMallocSignalMemory) == hipSuccess &&
                    hipExtMallocWithFlags((void **)&c->sigB1, 8, hipMallocSignalMemory) == hipSuccess) {
                    HIPCHK(c, hipMemset(c->sigB, 0, 8));
                    HIPCHK(c, hipMemset(c->sigB1, 0, 8));
                    c->handover_value = true;
                } else
                    (void)hipGetLastError();
            }
        }
        HIPCHK(c, hipEventCreateWithFlags(&c->evI, fl));
        HIPCHK(c, hipEventCreateWithFlags(&c->evX, fl));
        HIPCHK(c, hipEventCreateWithFlags(&c->evE, fl));
    }
    HIPCHK(c, hipEventCreate(&c->ev0));
    HIPCHK(c, hipEventCreate(&c->ev1));
    const size_t nd = slab_doubles(s), nm = mask_elems(s);
    HIPCHK(c, hipMalloc(&s.F, sizeof(double) * nd));
    HIPCHK(c, hipMemsetAsync(s.F, 0, sizeof(double) * nd, c->stream));
    HIPCHK(c, hipMalloc(&s.tmask, sizeof(int32_t) * nm));
    HIPCHK(c, hipMalloc(&s.umask, sizeof(int32_t) * nm));
    HIPCHK(c, hipMalloc(&s.iceumask, sizeof(int32_t) * nm));
    HIPCHK(c, hipMalloc(&s.cmask, nm));
    HIPCHK(c, hipMalloc(&s.tmphm, nm));
    HIPCHK(c, hipMemsetAsync(s.tmask, 0, sizeof(int32_t) * nm, c->stream));
    HIPCHK(c, hipMemsetAsync(s.umask, 0, sizeof(int32_t) * nm, c->stream));
    HIPCHK(c, hipMemsetAsync(s.iceumask, 0, sizeof(int32_t) * nm, c->stream));
    HIPCHK(c, hipMemsetAsync(s.cmask, 0, nm, c->stream));
    HIPCHK(c, hipMemsetAsync(s.tmphm, 0, nm, c->stream));
    s.ntx = (s.nxl + 2 + TILE_X - 1) / TILE_X;
    s.nty = (s.nyl + 2 + TILE_Y - 1) / TILE_Y;
    {
        const size_t nt = (size_t)s.ntx * s.nty;
        HIPCHK(c, hipMalloc(&c->tile_buf, 6 * nt));
        HIPCHK(c, hipMemsetAsync(c->tile_buf, 1, 6 * nt, c->stream));
        s.act_ice = c->tile_buf + 4 * nt;
        s.act_any = c->tile_buf + 5 * nt;
    }
    // (nblocks == 0: every block of this rank's columns was eliminated as land, ice_domain.F90:387-441 -- a slab of land that
    //  still serves its neighbours' ghost zones; nothing is gathered or scattered: the launches over blocks are skipped)
    HIPCHK(c, hipMalloc(&c->d_bd, sizeof(BlockDesc) * std::max(1, (int)g->nblocks)));
    if (g->nblocks) HIPCHK(c, hipMemcpyAsync(c->d_bd, c->bd.data(), sizeof(BlockDesc) * g->nblocks, hipMemcpyHostToDevice, c->stream));
    c->stage_n = (size_t)g->nblocks * g->ny_block * g->nx_block;
    HIPCHK(c, hipMalloc(&c->stage, sizeof(double) * std::max<size_t>(c->stage_n, 1)));

    // strips: 63 U columns x R U rows per wave.  Small slabs get short strips so that
    // the chip still sees enough waves.
    c->ncx = (s.nxl + 1 + STRIP_W - 1) / STRIP_W;
    {
        const char *e = getenv("EVPK_STRIP_ROWS");
        int R = e ? atoi(e) : 0;
        if (R <= 0) {
            const long long cells = (long long)s.nxl * s.nyl;
            R = cells >= 4000000 ? 16 : (cells >= 500000 ? 8 : 4);
        }
        c->R = std::max(1, std::min(R, 64));
    }
    c->nry = (s.nyl + 1 + c->R - 1) / c->R;
    {
        const size_t n1 = (size_t)c->ncx * ((s.nyl + 1 + std::min(c->R, 4) - 1) / std::min(c->R, 4));      // (tune_R1 goes down to R = 4)
        HIPCHK(c, hipMalloc(&c->d_flags, n1));
        HIPCHK(c, hipMalloc(&c->d_strips, sizeof(int) * n1));
    }
    HIPCHK(c, hipMalloc(&c->d_counts, sizeof(unsigned long long) * 4));
    c->ncx2 = (s.nxl + STRIP2_W - 1) / STRIP2_W;
    {
        const size_t n2 = (size_t)((s.nxl + 2 * (ZW_MAX - 2) + STRIP2_W - 1) / STRIP2_W) * (s.nyl + 2);   // any strip height >= 1, any zone width
        HIPCHK(c, hipMalloc(&c->d_flags2, n2));
        HIPCHK(c, hipMalloc(&c->d_strips2, sizeof(int) * n2));
        HIPCHK(c, hipMalloc(&c->d_strips2e, sizeof(int) * n2));
        HIPCHK(c, hipMalloc(&c->d_strips2i, sizeof(int) * n2));
        HIPCHK(c, hipMalloc(&c->d_tune, sizeof(unsigned int) * 64));
        c->R2 = c->R;
        c->nry2 = (s.nyl + 1 + c->R2 - 1) / c->R2;
    }
    {   // EVPK_OVERLAP=0 / 1 fixes the edge / interior split of the exchange launches; unset: the first evp (one-time
        // costs: connections, tuning) is not counted, the second runs with the split, the third without, and the faster
        // loop stays.  The choice only changes this rank's stream scheduling, not the order of its exchanges, so ranks
        // may decide differently.
        const char *e = getenv("EVPK_OVERLAP");
        c->overlap = !(e && atoi(e) == 0);
        c->ov_fixed = (e != nullptr);
    }
    // the pair kernel without the LDS prefetch was measured and not adopted: retired, see DESIGN.md
    { const char *e = getenv("EVPK_PREFETCH"); if (e && atoi(e) == 0) FAIL(c, "EVPK_PREFETCH=0 selects k_subcycle2, which was retired (last held by commit 11c5403)"); }
    // the tile kernel that rolls north through its strip was measured and not adopted: retired, see DESIGN.md
    {
        const char *e = getenv("EVPK_TILE");
        if (e && atoi(e) == 2) FAIL(c, "EVPK_TILE=2 selects k_subcycle2r, which was retired (last held by commit 2a9e752)");
        c->tile_force = e ? (atoi(e) != 0 ? 1 : 0) : -1;
    }
    { const char *e = getenv("EVPK_VERIFY_DELIVERY"); c->verify_delivery = e ? atoi(e) : 0; }
    { const char *e = getenv("EVPK_XFER_FUSED"); c->xfer_fused = !(e && atoi(e) == 0); }
    c->nsimd = 4 * prop.multiProcessorCount;

    // neighbours on the slab ring
    int lay[5];
    evpk_slab_layout(g->nx_global, c->nranks, g->rank, g->ew_boundary, i0, i1, lay);
    c->west = lay[0]; c->east = lay[1];
    {
        const char *fe = getenv("EVPK_FORCE_EXCHANGE");
        c->force_exchange = fe && atoi(fe) != 0;
        if (fe && atoi(fe) == 2 && c->xranks == 1) {
            // ... and EVPK_FORCE_EXCHANGE=2 routes that self-exchange through a ONE-rank RCCL communicator: ncclSend / ncclRecv
            // to itself inside a group and ncclAllGather, with the production buffers, counts and stream (tests: the RCCL
            // call path on a one-GPU box)
            ncclUniqueId u;
            NCCLCHK(c, ncclGetUniqueId(&u));
            NCCLCHK(c, ncclCommInitRank(&c->comm, 1, u, 0));
        }
    }
    const size_t eslot = (size_t)c->max_nf * (s.nyl + 2);
    HIPCHK(c, hipMalloc(&c->sendbuf, sizeof(double) * 2 * eslot));
    HIPCHK(c, hipMalloc(&c->recvbuf, sizeof(double) * 2 * eslot));
    HIPCHK(c, hipMemsetAsync(c->sendbuf, 0, sizeof(double) * 2 * eslot, c->stream));
    HIPCHK(c, hipMemsetAsync(c->recvbuf, 0, sizeof(double) * 2 * eslot, c->stream));
    c->sendW = c->sendbuf; c->sendE = c->sendbuf + eslot;      // re-pointed per call: [W edge | E edge], nf*(nyl+2) each
    c->recvE = c->recvbuf; c->recvW = c->recvbuf + eslot;      // [east ghost | west ghost]
    c->cslot = (size_t)25 * ZW_MAX * (s.nyl + 2);
    HIPCHK(c, hipMalloc(&c->cbuf, sizeof(double2) * 4 * c->cslot));
    HIPCHK(c, hipMemsetAsync(c->cbuf, 0, sizeof(double2) * 4 * c->cslot, c->stream));
    HIPCHK(c, hipMalloc(&c->d_zflags, (size_t)4 * (s.nyl + 2)));
    HIPCHK(c, hipMalloc(&c->d_zrows, sizeof(int) * 4 * (s.nyl + 2)));
    if (g->ns_boundary == EVPK_BND_TRIPOLE) {
        HIPCHK(c, hipMalloc(&c->foldbuf, sizeof(double) * (size_t)c->max_nf * 2 * s.nxg));
        HIPCHK(c, hipMemsetAsync(c->foldbuf, 0, sizeof(double) * (size_t)c->max_nf * 2 * s.nxg, c->stream));
    }

    // time-invariant planes
    struct { const double *h; int f; } gp[] = {
        {g->dxt, F_DXT}, {g->dyt, F_DYT}, {g->dxhy, F_DXHY}, {g->dyhx, F_DYHX}, {g->cxp, F_CXP}, {g->cyp, F_CYP},
        {g->cxm, F_CXM}, {g->cym, F_CYM}, {g->tinyarea, F_TINYAREA}, {g->tarear, F_TAREAR}, {g->tarea, F_TAREA},
        {g->uarea, F_UAREA}, {g->uarear, F_UAREAR}, {g->fcor, F_FCOR}};
    for (auto &e : gp) {
        if (!e.h) FAIL(c, "a grid plane pointer is NULL");
        if (upload_f(c, e.h, e.f)) return 1;
    }
    if (!g->tmask || !g->umask) FAIL(c, "tmask/umask is NULL");
    if (upload_m(c, g->tmask, s.tmask)) return 1;
    if (upload_m(c, g->umask, s.umask)) return 1;
    if (g->HTN && g->HTE) {
        // optional primary lengths: use them in place of the eight metric planes only if they reproduce those bit for bit
        if (upload_f(c, g->HTN, F_HTN) || upload_f(c, g->HTE, F_HTE)) return 1;
        c->have_lengths = true;
        const char *e = getenv("EVPK_COMPACT_METRICS");
        if (!(e && atoi(e) == 0)) {
            HIPCHK(c, hipMemsetAsync(c->d_tune, 0, sizeof(unsigned int), c->stream));
            hipLaunchKernelGGL(k_verify_metrics, dim3((s.nxl + 1 + 63) / 64, (s.nyl + 1 + 3) / 4), B2D, 0, c->stream, s, c->d_tune);
            unsigned int bad = 1;
            HIPCHK(c, hipMemcpyAsync(&bad, c->d_tune, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->compact = (bad == 0);
        }
    }
    if (!c->full_cover) {
        // cells of eliminated land blocks: give the areas a harmless non-zero value
        // (they are divisors in to_ugrid / to_tgrid; the reference never visits them)
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (const char *bf = getenv("EVPK_BAND_FUSED")) c->band_fused = atoi(bf) != 0;
    if (const char *ff = getenv("EVPK_FINISH_FUSED")) c->finish_fused = atoi(ff) != 0;
    if (const char *ds = getenv("EVPK_DEVICE_STRIPS")) c->dev_strips_env = atoi(ds) != 0;
    // the kernel of three subcycles per launch was measured and not adopted: retired, see DESIGN.md
    if (const char *tr = getenv("EVPK_TRIPLE")) if (atoi(tr) != 0) FAIL(c, "EVPK_TRIPLE=1 selects k_subcycle3w, which was retired (last held by commit 11c5403)");
    c->dbg_file = getenv("EVPK_DEBUG_CLOCKS");
    if (const char *pr = getenv("EVPK_PRIO")) c->prio = atoi(pr);
    if (const char *bl = getenv("EVPK_BAND_LAST")) c->band_last = atoi(bl) != 0 ? 1 : 0;
    HIPCHK(c, hipMalloc(&c->d_ns2, sizeof(int) * 2));
    HIPCHK(c, hipMemset(c->d_ns2, 0, sizeof(int) * 2));
    HIPCHK(c, hipHostMalloc((void **)&c->h_counts, sizeof(unsigned long long) * 4, hipHostMallocDefault));
    memset(c->h_counts, 0, sizeof(unsigned long long) * 4);
    const char *tk = getenv("EVPK_TIME_KERNELS");
    c->time_kernels = tk ? std::max(0, std::min(atoi(tk), 2)) : 1;
    // a multi-rank context without a unique id stays unconnected until evpk_connect (two-phase start)
    if (c->xranks == 1 || g->unique_id) return connect_impl(c, g->unique_id);
    return 0;
}

extern "C" int evpk_create(const evpk_geom *g, evpk_ctx **out) {
    if (!out) return 1;
    *out = nullptr;
    evpk_ctx *c = new evpk_ctx();
    if (create_impl(c, g)) {
        g_create_err = c->err;
        destroy_impl(c);
        return 1;
    }
    *out = c;
    return 0;
}

extern "C" int evpk_set_params(evpk_ctx *c, const evpk_params *p) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !p) return 1;
    if (p->ndte < 1 || !(p->dt > 0.0)) FAIL(c, "bad dt/ndte");
    DevParams &d = c->p;
    d.dt = p->dt; d.ndte = p->ndte; d.revp = p->revp; d.ecci = p->ecci; d.denom1 = p->denom1;
    d.arlx1i = p->arlx1i; d.brlx = p->brlx; d.cosw = p->cosw; d.sinw = p->sinw;
    d.rhow = p->rhow; d.rhoi = p->rhoi; d.rhos = p->rhos; d.gravit = p->gravit;
    d.a_min = p->a_min; d.m_min = p->m_min;
    d.tilt_from_slope = p->tilt_from_slope; d.wind_on_ugrid = p->wind_on_ugrid;
    d.kstrength = p->kstrength; d.krdg_partic = p->krdg_partic; d.krdg_redist = p->krdg_redist; d.ncat = p->ncat;
    d.mu_rdg = p->mu_rdg; d.Cf = p->Cf;
    d.sparse_io = p->sparse_io;
    if ((p->revised_evp != 0) != (p->revp == 1.0)) FAIL(c, "revised_evp and revp disagree");
    c->have_params = true;
    c->up_dirty = true;            // (rhoi / rhos enter the tile scan of the inputs)
    return 0;
}

extern "C" int evpk_upload(evpk_ctx *c, const evpk_step_in *in, const evpk_state *st) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !in) return 1;
    if (!c->have_params) FAIL(c, "evpk_set_params has not been called");
    if (!c->connected) FAIL(c, "evpk_connect has not been called (multi-rank context created without a unique id)");
    if (!st && !c->uploaded) FAIL(c, "the first evpk_upload needs the state");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    // sparse transfers (evpk_params.sparse_io, resident state, a prep behind us): aice / vice / vsno whole, the tiles they put
    // ice in -- or that were active at the previous evp -- for everything else
    const bool sparse = c->p.sparse_io && !st && c->uploaded && !c->fresh;
    const unsigned char *act = nullptr;
    if (sparse) {
        if (!c->io_raw) {
            HIPCHK(c, hipMalloc(&c->io_raw, (size_t)s.ntx * s.nty));
            HIPCHK(c, hipMalloc(&c->io_act, (size_t)s.ntx * s.nty));
        }
        if (!in->aice || !in->vice || !in->vsno) FAIL(c, "a required input pointer is NULL");
        // sparse_io = 1: aice, vice, vsno whole (one launch); = 2: aice alone -- vice and vsno are zero where aice is (the host's
        // promise: CICE's zap_small_areas / cleanup_itd keep it so) and travel in the active tiles like the other inputs
        const int aice_only = (c->p.sparse_io >= 2) ? 1 : 0;
        {
            XferBatch WB;
            WB.c = c;
            if (upload_fb(WB, in->aice, F_AICE, nullptr)) return 1;
            if (!aice_only && (upload_fb(WB, in->vice, F_VICE, nullptr) || upload_fb(WB, in->vsno, F_VSNO, nullptr))) return 1;
            if (WB.flush()) return 1;
        }
        hipLaunchKernelGGL(k_io_tiles, grid2d(s, B2D), B2D, 0, c->stream, s, c->p, c->io_raw, aice_only);
        hipLaunchKernelGGL(k_io_tiles_dilate, dim3((s.ntx + 63) / 64, s.nty), dim3(64), 0, c->stream, s, (const unsigned char *)c->io_raw, c->io_act);
        HIPCHK(c, hipGetLastError());
        act = c->io_act;
    }
    c->io_sparse_now = sparse;
    c->up_dirty = true;
    const bool vsparse = sparse && c->p.sparse_io >= 2;
    struct { const double *h; int f; bool need; } ip[] = {
        {in->aice, F_AICE, true}, {in->vice, F_VICE, true}, {in->vsno, F_VSNO, true}, {in->aice_init, F_AICE_INIT, true},
        {in->uocn, F_UOCN, true}, {in->vocn, F_VOCN, true}, {in->Cdn_ocn, F_CW, true}, {in->strength, F_STRENGTH, false},
        {in->ss_tltx, F_SSTLTX, c->p.tilt_from_slope != 0}, {in->ss_tlty, F_SSTLTY, c->p.tilt_from_slope != 0},
        // wind: either T-grid stress (t2ugrid_vector) or U-grid stress (ACCESS); both land in STRAIRXT/YT
        {c->p.wind_on_ugrid ? in->strax : in->strairxT, F_STRAIRXT, true},
        {c->p.wind_on_ugrid ? in->stray : in->strairyT, F_STRAIRYT, true}};
    XferBatch UB;
    UB.c = c;
    for (auto &e : ip) {
        if (!e.h) { if (e.need) FAIL(c, "a required input pointer is NULL"); continue; }
        if (sparse && (e.f == F_AICE || (!vsparse && (e.f == F_VICE || e.f == F_VSNO)))) continue;      // (uploaded whole above)
        if (upload_fb(UB, e.h, e.f, act)) return 1;
    }
    if (UB.flush()) return 1;
    c->strength_dev = (in->strength == nullptr);
    if (c->strength_dev && c->p.kstrength == 1) {
        // thickness distribution for ice_strength on the device: (nx_block, ny_block, ncat, nblocks) arrays, one plane per category
        const int ncat = c->p.ncat;
        if (ncat < 1 || ncat > MAXCAT) FAIL(c, "ice_strength on the device: ncat = %d not in 1..%d", ncat, MAXCAT);
        if (!in->aicen || !in->vicen || !in->aice0) FAIL(c, "strength == NULL with kstrength == 1 needs aicen, vicen and aice0");
        const size_t np = mask_elems(s), nblk = (size_t)c->nyb * c->nxb;
        if (c->itd_ncat != ncat) {
            if (c->itd) (void)hipFree(c->itd);
            if (c->stage_itd) (void)hipFree(c->stage_itd);
            c->itd = c->stage_itd = nullptr;
            HIPCHK(c, hipMalloc(&c->itd, sizeof(double) * np * (2 * ncat + 1)));
            HIPCHK(c, hipMemsetAsync(c->itd, 0, sizeof(double) * np * (2 * ncat + 1), c->stream));
            HIPCHK(c, hipMalloc(&c->stage_itd, sizeof(double) * c->stage_n * ncat));
            c->itd_ncat = ncat;
        }
        const dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
        const double *hosts[3] = {in->aicen, in->vicen, in->aice0};
        for (int a = 0; a < 3; a++) {
            const int nc = a < 2 ? ncat : 1;
            const double *src = (const double *)mapped_alias(hosts[a], sizeof(double) * c->stage_n * nc);
            if (!src) {
                HIPCHK(c, hipMemcpyAsync(c->stage_itd, hosts[a], sizeof(double) * c->stage_n * nc, hipMemcpyHostToDevice, c->stream));
                src = c->stage_itd;
            }
            for (int n = 0; n < nc; n++)
                LAUNCH_BLOCKS(k_gather_plane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, src + (size_t)n * nblk, (size_t)nc * nblk,
                                   c->itd + (size_t)(a * ncat + n) * np);
        }
        HIPCHK(c, hipGetLastError());
    }
    if (!st) {      // inputs only: the prognostic state stays resident on the device
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->prepped = false;
        return 0;
    }
    if (!st->uvel || !st->vvel || !st->iceumask) FAIL(c, "uvel/vvel/iceumask is NULL");
    if (upload_fb(UB, st->uvel, F_STATE0 + S_U, nullptr)) return 1;
    if (upload_fb(UB, st->vvel, F_STATE0 + S_V, nullptr)) return 1;
    for (int q = 0; q < 4; q++) {
        if (!st->stressp[q] || !st->stressm[q] || !st->stress12[q]) FAIL(c, "a stress pointer is NULL");
        if (upload_fb(UB, st->stressp[q], F_STATE0 + S_SP + q, nullptr)) return 1;
        if (upload_fb(UB, st->stressm[q], F_STATE0 + S_SM + q, nullptr)) return 1;
        if (upload_fb(UB, st->stress12[q], F_STATE0 + S_S12 + q, nullptr)) return 1;
    }
    if (upload_m(c, st->iceumask, s.iceumask)) return 1;
    // strintx/y, strocnx/y are inout in evp_prep2 (kept where iceumask stays true until the loop rewrites them)
    if (upload_fb(UB, st->strintx, F_STRINTX, nullptr) || upload_fb(UB, st->strinty, F_STRINTY, nullptr)) return 1;
    if (upload_fb(UB, st->strocnx, F_STROCNX, nullptr) || upload_fb(UB, st->strocny, F_STROCNY, nullptr)) return 1;
    if (UB.flush()) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->cur = 0;
    c->uploaded = true;
    c->prepped = false;
    c->fresh = true;
    return 0;
}

// Strip height of the pair kernels.  The kernel's run time is quantised in "rounds" of resident workgroups
// (2 per CU): a launch with slightly more workgroups than fit pays a whole extra round, while tall strips
// waste less on the three redundant stage-1 rows.  Count the active strips for a few heights and take the
// cheapest  rounds x (R+5).  Re-tuned when the active area changed by more than 5 %.
static int tune_R2(evpk_ctx *c) {
    const char *e = getenv("EVPK_STRIP_ROWS");
    if (e && atoi(e) > 0) {
        c->tile_mode = (c->tile_force == 1);
        c->R2 = std::max(1, std::min(atoi(e), c->tile_mode ? 13 : 64)); c->nry2 = (c->s.nyl + 1 + c->R2 - 1) / c->R2;
        return 0;
    }
    // icellt of this prep is not known yet on the host; use the previous one as the trigger
    if (c->tuned_icellt >= 0 && std::llabs(c->icellt - c->tuned_icellt) * 20 <= c->tuned_icellt) return 0;
    static const int cand[] = {2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32, 36, 40, 48};
    static const int tcand[] = {2, 3, 4, 5, 6, 8, 10, 13};        // tile heights of k_subcycle2t: R + 3 <= 16 waves per workgroup
    static const int rcand[] = {11, 17, 23, 29, 35, 47, 59};      // strip heights of the retired rolling tile kernel, see below: R + 3 = 8 + 6 k
    const int ncand = (int)(sizeof(cand) / sizeof(cand[0])), ntc = (int)(sizeof(tcand) / sizeof(tcand[0])), nrc = (int)(sizeof(rcand) / sizeof(rcand[0]));
    Slab &s = c->s;
    HIPCHK(c, hipMemsetAsync(c->d_tune, 0, sizeof(unsigned int) * 64, c->stream));
    const int cyc = (c->ew == EVPK_BND_CYCLIC && !c->zone_mode) ? 1 : 0;
    const int G = c->zone_mode ? c->zW - 2 : 0;
    for (int k = 0; k < ncand + ntc + nrc; k++) {
        const int R = k < ncand ? cand[k] : (k < ncand + ntc ? tcand[k - ncand] : rcand[k - ncand - ntc]), nry = (s.nyl + 1 + R - 1) / R, tot = c->ncx2 * nry;
        hipLaunchKernelGGL(k_strip_flags2, dim3((tot + 3) / 4), dim3(256), 0, c->stream, s, c->ncx2, nry, R, cyc, G,
                           (unsigned char *)nullptr, c->d_tune + k);
    }
    unsigned int cnt[64];
    HIPCHK(c, hipMemcpyAsync(cnt, c->d_tune, sizeof(unsigned int) * 64, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // Both variants in microseconds per launch, from measurements on MI355X (profiles/r02_*/tile_ab.txt): one wave alone on
    // its SIMD takes ~5.3 us per march step (a dependent fp64 chain), ~7.5 us when a second wave shares the SIMD; the first
    // R + 3 - 1.5 steps of a strip are full ones.  A tile workgroup of R + 3 waves sits on ONE CU, ceil((R+3)/4) waves per
    // SIMD, ~3.6 us per wave-row when enough waves overlap; a workgroup that fills the CU alone (more than 8 waves) has
    // nothing to hide its three barriers behind.
    double best = 1e300, bestT = 1e300;
    int bestR = c->R2, bestH = 5;
    for (int k = 0; k < ncand; k++) {
        const long long nwg = (cnt[k] + 3) / 4;
        if (nwg == 0) continue;
        const long long rounds = (nwg + c->slots2 - 1) / c->slots2;
        const double per_round = (double)cnt[k] / (double)rounds;
        const double step_us = per_round > (double)c->nsimd ? 7.5 : 5.3;
        const double cost = (double)rounds * ((cand[k] + 1.5) * step_us + 4.0);
        if (cost < best * 0.999) { best = cost; bestR = cand[k]; }
    }
    for (int k = ntc - 1; k >= 0; k--) {
        const unsigned int nt = cnt[ncand + k];
        if (nt == 0) continue;
        const int nw = tcand[k] + 3;
        const double per_simd = std::max((double)((nw + 3) / 4), (double)nt * nw / (double)c->nsimd * (nw > 8 ? 1.35 : 1.0));
        const double cost = 3.6 * per_simd + 6.0;
        if (cost < bestT * 0.999) { bestT = cost; bestH = tcand[k]; }
    }
    // The estimate of a RETIRED kernel: the tile kernel of round 5 that rolled north through a strip in passes of six rows, eight
    // waves per workgroup, without the three redundant rows per tile (four barriers per pass).  It was measured and not adopted
    // (profiles/r05_v1/roll_ab.txt: 26 % fewer rows computed, the same rows per microsecond -- the small slabs are bound by the
    // latency of a workgroup's phase chain, not by the arithmetic) and the tuner never launched it, but its estimate has always been
    // part of the comparison below and still tips the choice to k_subcycle2t on mid-size slabs (1440x1080 tripole: march 52.8,
    // tile 53.0, this term 43.0 us).  Kept because removing it changes which kernel runs there; to be replaced only together with
    // a measurement on those grids, as ADVICE.md asks.  It feeds tile_mode only: R2 is bestH or bestR.
    constexpr int roll_nw = 8;      // waves per workgroup of that kernel
    double bestRo = 1e300;
    for (int k = 0; k < nrc; k++) {
        const unsigned int nt = cnt[ncand + ntc + k];
        if (nt == 0 || rcand[k] + 3 > s.nyl + 8) continue;
        const int passes = 1 + (rcand[k] + 3 - roll_nw) / (roll_nw - 2);
        const double per_simd = std::max(2.0 * passes, (double)nt * (rcand[k] + 3) / (double)c->nsimd);
        const double cost = 3.6 * per_simd + 6.0 + 0.6 * passes;
        if (cost < bestRo * 0.999) bestRo = cost;
    }
    c->tile_mode = c->tile_force >= 0 ? (c->tile_force == 1) : (std::min(bestT, bestRo) < best);
    if (best > 1e299 && bestT > 1e299) c->tile_mode = false;
    c->R2 = c->tile_mode ? bestH : bestR;
    c->nry2 = (s.nyl + 1 + c->R2 - 1) / c->R2;
    c->tuned_icellt = -2;      // set from the counts of this prep below
    return 0;
}

// Strip list of the one-subcycle kernel (and, when the two-subcycle kernel is off, the active-cell counts): flags on the
// device, compaction on the host.  Called by evpk_prep when only that kernel exists, else on first use after a prep.
// Strip height of the one-subcycle kernels when they ARE the loop (eap, EVPK_DOUBLE=0) on a large slab.  A launch runs its strips in
// rounds of resident workgroups (four strips each, four workgroups per CU at 128 VGPRs: 4 096 strips); measured for k_eap_sub at
// 3600x2700 (round 4, EVPK_STRIP_ROWS sweep): R = 16, the fixed default until then, 47.2 ms per eap with 2 816 strips = 2.75 waves per
// SIMD; R = 11 41.8 ms (3 850 strips, 3.76 waves per SIMD: the latency-bound corner chains want every wave they can get); R = 10
// 52.9 ms (4 240 strips: a second round).  A march step takes ~(2.2 + waves per SIMD) x 4.9 us, so the cheapest
// rounds x (R + 1) x (2.2 + 4 x fill) wins.  Re-tuned when the active area changed by more than 5 %.
static int tune_R1(evpk_ctx *c) {
    Slab &s = c->s;
    if (getenv("EVPK_STRIP_ROWS") || (long long)s.nxl * s.nyl < 500000 || !(c->eap || !c->use_double)) return 0;
    if (c->tuned1_icellt >= 0 && std::llabs(c->icellt - c->tuned1_icellt) * 20 <= c->tuned1_icellt) return 0;
    static const int cand[] = {4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 22, 24, 26, 28, 32, 36, 40, 48};
    const int ncand = (int)(sizeof(cand) / sizeof(cand[0]));
    HIPCHK(c, hipMemsetAsync(c->d_tune, 0, sizeof(unsigned int) * 32, c->stream));
    for (int k = 0; k < ncand; k++) {
        const int R = cand[k], nry = (s.nyl + 1 + R - 1) / R, tot = c->ncx * nry;
        hipLaunchKernelGGL(k_strip_flags, dim3((tot + 3) / 4), dim3(256), 0, c->stream, s, c->ncx, nry, R, (unsigned char *)nullptr,
                           (unsigned long long *)nullptr, c->d_tune + k);
    }
    unsigned int cnt[32];
    HIPCHK(c, hipMemcpyAsync(cnt, c->d_tune, sizeof(unsigned int) * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double slots = 4.0 * c->nsimd;          // strips resident at four waves per SIMD
    double best = 1e300;
    int bestR = c->R;
    for (int k = 0; k < ncand; k++) {
        if (cnt[k] == 0) continue;
        const double rounds = std::ceil(cnt[k] / slots), fill = cnt[k] / (rounds * slots);
        const double cost = rounds * (cand[k] + 1) * (2.2 + 4.0 * fill);
        if (cost < best * 0.999) { best = cost; bestR = cand[k]; }
    }
    c->R = bestR;
    c->nry = (s.nyl + 1 + c->R - 1) / c->R;
    c->tuned1_icellt = c->icellt > 0 ? c->icellt : -1;      // (the first evp tunes before icellt is known: tune once more then)
    return 0;
}

static int strips1(evpk_ctx *c) {
    if (c->strips1_valid) return 0;
    if (tune_R1(c)) return 1;
    Slab &s = c->s;
    const int ns_tot = c->ncx * c->nry;
    unsigned long long *d_cnt = c->use_double ? c->d_counts + 2 : c->d_counts;      // (the counts of prep stay untouched)
    HIPCHK(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * 2, c->stream));
    hipLaunchKernelGGL(k_strip_flags, dim3((ns_tot + 3) / 4), dim3(256), 0, c->stream, s, c->ncx, c->nry, c->R, c->d_flags, d_cnt);
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned char> flags(ns_tot);
    HIPCHK(c, hipMemcpyAsync(flags.data(), c->d_flags, ns_tot, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> list;
    list.reserve(ns_tot);
    for (int k = 0; k < ns_tot; k++) if (flags[k]) list.push_back(k);
    c->nstrips = (int)list.size();
    if (c->nstrips) HIPCHK(c, hipMemcpy(c->d_strips, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    c->strips1_valid = true;
    return 0;
}

extern "C" int evpk_prep(evpk_ctx *c) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c) return 1;
    if (!c->uploaded) FAIL(c, "evpk_upload has not been called");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const dim3 g2 = grid2d(s, B2D);
    const int SA = c->cur ? F_STATE1 : F_STATE0, SB = c->cur ? F_STATE0 : F_STATE1;   // current / other state buffer
    // evp_prep1 + zero diagnostics (ice_dyn_evp.F90:171-203)
    const int fresh = c->fresh ? 1 : 0;
    const size_t ntile = (size_t)s.ntx * s.nty;
    unsigned char *prev_ice = c->tile_buf + (size_t)(c->tile_cur ? 0 : 2) * ntile, *prev_dat = prev_ice + ntile;
    s.tile_ice = c->tile_buf + (size_t)(c->tile_cur ? 2 : 0) * ntile;
    s.tile_dat = s.tile_ice + ntile;
    c->tile_cur ^= 1;
    if (c->up_dirty) {      // the host's inputs changed since the last scan: which tiles hold anything at all
        if (!c->up_dat) HIPCHK(c, hipMalloc(&c->up_dat, ntile));
        hipLaunchKernelGGL(k_up_tiles, g2, B2D, 0, c->stream, s, c->p, c->up_dat);
        c->up_dirty = false;
    }
    hipLaunchKernelGGL(k_prep1a, g2, B2D, 0, c->stream, s, c->p, fresh, (const unsigned char *)c->up_dat);
    hipLaunchKernelGGL(k_tile_dilate, dim3((s.ntx + 63) / 64, s.nty), dim3(64), 0, c->stream, s, (const unsigned char *)prev_ice,
                       (const unsigned char *)prev_dat, fresh);
    hipLaunchKernelGGL(k_prep1b, g2, B2D, 0, c->stream, s);
    if (halo(c, F_ICETM, 1, false, false, 0.0)) return 1;                         // :210-211
    if (c->strength_dev) {                                                        // ice_strength, :291-301
        // (five categories -- the reference's default -- at compile time: work arrays in registers, no scratch memory; Hibler's
        //  formula uses no work arrays at all)
        if (c->p.kstrength != 1 || c->p.ncat == 5) { hipLaunchKernelGGL(k_ice_strength<5>, g2, B2D, 0, c->stream, s, c->p, (const double *)c->itd); }
        else { hipLaunchKernelGGL(k_ice_strength<0>, g2, B2D, 0, c->stream, s, c->p, (const double *)c->itd); }
    }
    // to_ugrid (:218-219) and t2ugrid_vector (:240-241; the T-grid wind sits in the work planes)
    if (!c->p.wind_on_ugrid && halo(c, F_WORK1, 2, false, true, 0.0)) return 1;
    hipLaunchKernelGGL(k_to_ugrid4, g2, B2D, 0, c->stream, s, c->p.wind_on_ugrid ? 0 : 1);
    // evp_prep2 (:247-308); strength is an input (ice_strength, :291-301)
    hipLaunchKernelGGL(k_prep2, g2, B2D, 0, c->stream, s, c->p, fresh, c->cur);
    // (x-slabs with ghost zones: the zone exchange below carries the E-W ghost columns of strength and of the state)
    const bool zm = c->use_double && (c->nranks > 1 || c->force_exchange);
    if (halo(c, F_STRENGTH, 1, false, false, 0.0, -1, nullptr, zm)) return 1;     // :311-312
    if (halo(c, SA + S_U, 2, true, true, 0.0, -1, nullptr, zm)) return 1;         // :314-315
    {   // the top physical row may have been rewritten by a tripole fold, the ring by the halo: mirror into buffer 1
        const int nring = 2 * (s.nxl + 2) + 2 * (s.nyl + 2);
        hipLaunchKernelGGL(k_ring_copy, dim3((nring + 127) / 128), dim3(128), 0, c->stream, s, SA + S_U, SB + S_U, 2);
        if (c->ns == EVPK_BND_TRIPOLE)
            hipLaunchKernelGGL(k_row_copy, dim3((s.nxl + 2 + 127) / 128), dim3(128), 0, c->stream, s, SA + S_U, SB + S_U, 2, s.nyl);
    }
    if (c->band_mode)       // inactive cells of the scratch state keep the values they have at the start of the loop
        hipLaunchKernelGGL(k_rows_copy, dim3((s.nxl + 2 + 127) / 128, 6), dim3(128), 0, c->stream, s, SA + S_U, (int)(F_STATE2 + S_U), 2,
                           s.nyl - 4, s.nyl + 1);
    c->fresh = false;
    c->zone_mode = zm;
    const int G = c->zone_mode ? c->zW - 2 : 0;
    c->ncx2 = (s.nxl + 2 * G + STRIP2_W - 1) / STRIP2_W;
    c->zcompact = false;
    std::vector<unsigned char> zflags;
    if (c->zone_mode) {
        // ghost zones for the pair kernels: every plane they read, the current state and the masks, all rows, once per evp
        PairList pl = state_pairs(SA);
        const int per_evp[] = {F_TINYAREA /* + strength */, F_VRELC, F_UOCN, F_FORCEX, F_UMASSDTI, F_UVEL_INIT};
        const int once[] = {F_CXP, F_CXM, F_DXT, F_DXHY, F_HTN};        // grid metrics: the first evp only
        for (int f : per_evp) pl.p[pl.n++] = f >> 1;
        if (!c->zone_metrics_done)
            for (int f : once) pl.p[pl.n++] = f >> 1;
        c->zone_metrics_done = true;
        pl.with_cmask = 1;
        if (exchange_cols(c, pl, false)) return 1;
        // the other state buffer starts from the same zone image: cells no kernel writes are alike in both for good
        const int nz = 2 * c->zW * (s.nyl + 2);
        hipLaunchKernelGGL(k_zone_copy, dim3((nz + 255) / 256), dim3(256), 0, c->stream, s, c->zW, SA, SB, NSTATE / 2);
        if (!c->band_mode) {      // (tripole: the fold rewrites the top rows of every column, active or not)
            hipLaunchKernelGGL(k_zone_rows, dim3((s.nyl + 2 + 127) / 128), dim3(128), 0, c->stream, s, c->zW, c->d_zflags);
            zflags.resize((size_t)4 * (s.nyl + 2));
            HIPCHK(c, hipMemcpyAsync(zflags.data(), c->d_zflags, zflags.size(), hipMemcpyDeviceToHost, c->stream));
        }
        c->zone_left = c->zM;
        c->inner_ok = true;
        if (c->xband) {
            // the mirror slab: what band_pair reads of the mirror rank's rows N-3 .. N+1 -- metrics, strength, the stepu inputs,
            // the masks (once per evp) and the state
            XbList L{};
            for (int f : {(int)F_CXP, (int)F_CXM, (int)F_DXT, (int)F_DXHY, (int)F_TINYAREA, (int)F_VRELC, (int)F_UOCN, (int)F_FORCEX, (int)F_UMASSDTI,
                          (int)F_UVEL_INIT, (int)F_TAREAR, (int)F_HTN})
                L.f[L.np++] = f & ~1;
            if (xband_swap(c, L, s.nyl - c->m.nyl, 0, c->m.nyl + 2, 1, c->stream)) return 1;
            if (xband_state(c, SA, c->stream)) return 1;
            c->m_need = 0;
        }
    }
    // active strips.  The list of the one-subcycle kernel is only built when that kernel is going to run (odd ndte, EVPK_DOUBLE=0,
    // a partial evpk_subcycle call): strips1() below; the cell counts then come from the two-subcycle kernel's flag pass.
    HIPCHK(c, hipMemsetAsync(c->d_counts, 0, sizeof(unsigned long long) * 2, c->stream));
    c->strips1_valid = false;
    if (!c->use_double && strips1(c)) return 1;
    if (c->use_double && tune_R2(c)) return 1;
    const int ns_tot2 = c->ncx2 * c->nry2;
    // one rank, or x-slab ranks on a tripole grid (no edge / interior lists, no row lists of the zone windows to make on the host)
    c->dev_strips = c->dev_strips_env && c->use_double &&
                    ((!c->zone_mode && c->nranks == 1 && !c->force_exchange) || (c->zone_mode && c->band_mode));
    if (c->dev_strips) {
        // flags, ordered compaction and counts on the device; nothing comes back before the loop has run (subcycle_impl)
        hipLaunchKernelGGL(k_strip_flags2, dim3((ns_tot2 + 3) / 4), dim3(256), 0, c->stream, s, c->ncx2, c->nry2, c->R2,
                           (c->ew == EVPK_BND_CYCLIC && !c->zone_mode) ? 1 : 0, G, c->d_flags2, (unsigned int *)nullptr, c->d_counts);
        hipLaunchKernelGGL(k_compact_strips, dim3(1), dim3(1024), 0, c->stream, (const unsigned char *)c->d_flags2, ns_tot2, c->d_strips2, c->d_ns2);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_counts, c->d_counts, sizeof(unsigned long long) * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_counts + 2, c->d_ns2, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        c->ns_tot2_cur = ns_tot2;
        c->nstrips2 = ns_tot2;            // the launches cover the upper bound; the true number replaces it after the loop
        c->counts_pending = true;         // (evpk_get_stats before the loop synchronises and reads them)
        c->nstrips2e = c->nstrips2i = 0;
        c->ksub = 0;
        c->prepped = true;
        c->evp_count++;
        return 0;
    }
    std::vector<unsigned char> flags2(c->use_double ? ns_tot2 : 0);
    unsigned long long cnt[2] = {0, 0};
    if (c->use_double) {
        hipLaunchKernelGGL(k_strip_flags2, dim3((ns_tot2 + 3) / 4), dim3(256), 0, c->stream, s, c->ncx2, c->nry2, c->R2,
                           (c->ew == EVPK_BND_CYCLIC && !c->zone_mode) ? 1 : 0, G, c->d_flags2, (unsigned int *)nullptr, c->d_counts);
        HIPCHK(c, hipMemcpyAsync(flags2.data(), c->d_flags2, ns_tot2, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(cnt, c->d_counts, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> list2;
    if (c->use_double) {
        for (int k = 0; k < ns_tot2; k++) if (flags2[k]) list2.push_back(k);
        c->nstrips2 = (int)list2.size();
        if (c->nstrips2) HIPCHK(c, hipMemcpyAsync(c->d_strips2, list2.data(), sizeof(int) * list2.size(), hipMemcpyHostToDevice, c->stream));
        // interior strips neither read a ghost zone nor write a column the neighbours are sent (1..zW, nxl-zW+1..nxl):
        // lane 0 of strip cx sits at column x0 = cx*61 - G, the strip reads x0-1 .. x0+63 and stores x0+1 .. x0+61.
        // The edge strips run first, the interior overlaps the exchange.
        std::vector<int> le, li;
        if (c->zone_mode && (c->overlap || !c->ov_fixed) && !c->band_mode)       // (only the split launches of x-slabs use the two lists)
            for (int k : list2) {
                const int x0 = (k % c->ncx2) * STRIP2_W - G;
                if (x0 >= c->zW && x0 <= s.nxl - c->zW - STRIP2_W) li.push_back(k); else le.push_back(k);
            }
        c->nstrips2e = (int)le.size(); c->nstrips2i = (int)li.size();
        if (c->nstrips2e) HIPCHK(c, hipMemcpyAsync(c->d_strips2e, le.data(), sizeof(int) * le.size(), hipMemcpyHostToDevice, c->stream));
        if (c->nstrips2i) HIPCHK(c, hipMemcpyAsync(c->d_strips2i, li.data(), sizeof(int) * li.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));      // the host vectors go out of scope
    }
    if (!zflags.empty()) {          // compacted row lists of the four zone windows
        const int rows = s.nyl + 2;
        std::vector<int> zl((size_t)4 * rows, 0);
        for (int w = 0; w < 4; w++) {
            int n = 0;
            for (int j = 0; j < rows; j++) if (zflags[(size_t)w * rows + j]) zl[(size_t)w * rows + n++] = j;
            c->zn[w] = n;
        }
        HIPCHK(c, hipMemcpyAsync(c->d_zrows, zl.data(), sizeof(int) * zl.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->zcompact = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (xp_check(c)) return 1;
    c->icellt = (long long)cnt[0];
    c->icellu = (long long)cnt[1];
    if (c->tuned_icellt == -2) c->tuned_icellt = c->icellt;
    c->ksub = 0;
    c->prepped = true;
    c->evp_count++;
    return 0;
}

// ---- EAP (source/ice_dyn_eap.F90), SURVEY S8 row f-4 -------------------------------------------------------------------------
extern "C" int evpk_eap_init(evpk_ctx *c, int32_t nx_yield, int32_t ny_yield, int32_t na_yield, const double *s11r, const double *s12r,
                             const double *s22r, const double *s11s, const double *s12s, const double *s22s) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !s11r || !s12r || !s22r || !s11s || !s12s || !s22s) return 1;
    if (nx_yield < 2 || ny_yield < 2 || na_yield < 2) FAIL(c, "evpk_eap_init: table extents %d x %d x %d", nx_yield, ny_yield, na_yield);
    if (!c->connected) FAIL(c, "evpk_eap_init: the context is not connected yet (evpk_connect)");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nt = (size_t)nx_yield * ny_yield * na_yield, np = mask_elems(s);
    if (c->eap_tab) (void)hipFree(c->eap_tab);
    c->eap_tab = nullptr;
    HIPCHK(c, hipMalloc(&c->eap_tab, sizeof(double) * 8 * nt));
    {   // entry q = {s11r, s12r, s22r, s11s, s12s, s22s, 0, 0}[q]: see EapDev
        const double *src[6] = {s11r, s12r, s22r, s11s, s12s, s22s};
        std::vector<double> inter(8 * nt, 0.0);
        for (size_t q = 0; q < nt; q++)
            for (int t = 0; t < 6; t++) inter[8 * q + t] = src[t][q];
        HIPCHK(c, hipMemcpy(c->eap_tab, inter.data(), sizeof(double) * 8 * nt, hipMemcpyHostToDevice));
    }
    c->E.tabs = c->eap_tab; c->E.nt = nt;
    c->E.nxy = nx_yield; c->E.nyy = ny_yield; c->E.nay = na_yield;
    c->E.invsin = eap_invsin();
    eap_set_steps(c->E);
    if (!c->eap_pool) {
        HIPCHK(c, hipMalloc(&c->eap_pool, sizeof(double) * EAP_NPLANES * np));
        HIPCHK(c, hipMemsetAsync(c->eap_pool, 0, sizeof(double) * EAP_NPLANES * np, c->stream));
        c->E.pool = c->eap_pool; c->E.np = np;
        for (int k = 0; k < 4; k++)      // init_eap (:529-551): isotropic structure tensor
            hipLaunchKernelGGL(k_fill_mplane, grid2d(s, B2D), B2D, 0, c->stream, s, c->E.a11(k), 0.5);
        hipLaunchKernelGGL(k_eap_angles, grid2d(s, B2D), B2D, 0, c->stream, s, c->E);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->eap = true;
    return 0;
}

static double *eap_member(evpk_ctx *c, int q) {       // the planes in the order of evpk_eap_state's members
    return q < 4 ? c->E.a11(q) : q < 8 ? c->E.a12(q - 4) : c->E.hist(q - 8);
}

extern "C" int evpk_eap_upload(evpk_ctx *c, const evpk_eap_state *st) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !st) return 1;
    if (!c->eap) FAIL(c, "evpk_eap_upload: evpk_eap_init has not been called");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nblk = (size_t)c->nyb * c->nxb, n = (size_t)c->nblocks * nblk;
    const dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
    for (int q = 0; q < 8; q++) {
        const double *h = q < 4 ? st->a11_c[q] : st->a12_c[q - 4];
        if (!h) continue;
        const double *dev = (const double *)mapped_alias(h, sizeof(double) * n);
        if (!dev) {
            HIPCHK(c, hipMemcpyAsync(c->stage, h, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
            dev = c->stage;
        }
        LAUNCH_BLOCKS(k_gather_plane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, dev, nblk, eap_member(c, q));
        HIPCHK(c, hipStreamSynchronize(c->stream));      // (the staging buffer is reused by the next array)
    }
    hipLaunchKernelGGL(k_eap_angles, grid2d(s, B2D), B2D, 0, c->stream, s, c->E);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int evpk_eap_download(evpk_ctx *c, evpk_eap_state *st) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !st) return 1;
    if (!c->eap) FAIL(c, "evpk_eap_download: evpk_eap_init has not been called");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->nblocks * c->nyb * c->nxb;
    const dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
    double *host[19] = {st->a11_c[0], st->a11_c[1], st->a11_c[2], st->a11_c[3], st->a12_c[0], st->a12_c[1], st->a12_c[2], st->a12_c[3],
                        st->a11, st->a12, st->e11, st->e12, st->e22, st->yieldstress11, st->yieldstress12, st->yieldstress22, st->s11, st->s12, st->s22};
    for (int q = 0; q < 19; q++) {
        if (!host[q]) continue;
        // T-cell fields: the physical cells and the N / E ghost T cells the reference computes too (ice_dyn_shared.F90:528-537)
        bool hostmem = false;
        if (double *dst = (double *)mapped_alias(host[q], sizeof(double) * n, &hostmem)) {
            LAUNCH_BLOCKS(k_scatter_mplane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)eap_member(c, q), dst, (int)MODE_NE);
            if (c->verify_delivery && hostmem) {
                HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->stage, (int)DV_SENTINEL32, 2 * n, c->stream));
                LAUNCH_BLOCKS(k_scatter_mplane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)eap_member(c, q), c->stage, (int)MODE_NE);
                HIPCHK(c, hipGetLastError());
                if (verify_plane(c, host[q], sizeof(double), n, q, "eap member")) return 1;
            }
            continue;
        }
        HIPCHK(c, hipMemcpyAsync(c->stage, host[q], n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        LAUNCH_BLOCKS(k_scatter_mplane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)eap_member(c, q), c->stage, (int)MODE_NE);
        HIPCHK(c, hipMemcpyAsync(host[q], c->stage, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// the per-call counters of evpk_get_stats: zero at the start of every subcycle call, whichever loop runs it
static void reset_call_counters(evpk_ctx *c) {
    c->kernel_ms = c->kernel2_ms = 0.f;
    c->kernel_launches = c->double_launches = 0;
    c->kernel_timed = c->kernel2_timed = 0;
    c->bound_updates = 0; c->bound_timed = 0; c->bound_ms = 0.f;
    c->xb_swaps = 0; c->zone_exchanges = 0; c->zone_bytes = 0;
}

// the subcycle loop of eap(dt) (ice_dyn_eap.F90:345-447): stress_eap, stepu, [stepa], velocity halo -- in place in the current buffer
static int eap_subcycle(evpk_ctx *c, int32_t nsub) {
    Slab &s = c->s;
    const int SB = c->cur ? F_STATE1 : F_STATE0;
    const dim3 gT((s.nxl + 1 + 63) / 64, (s.nyl + 1 + 3) / 4), gU((s.nxl + 63) / 64, (s.nyl + 3) / 4);
    const double dte = c->p.dt / (double)c->p.ndte, dtei = 1.0 / dte;        // ice_dyn_shared.F90:209-210
    reset_call_counters(c);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (c->ksub == 0) hipLaunchKernelGGL(k_eap_reset, grid2d(s, B2D), B2D, 0, c->stream, s, c->E);
    for (int n = 0; n < nsub; n++) {
        const int ksub = c->ksub + 1;
        const int hist = (ksub == c->p.ndte || n == nsub - 1) ? 1 : 0;      // the history fields of the call's last subcycle are the ones that can be seen
        with_bool(ksub == c->p.ndte, [&](auto LAST) {
            hipLaunchKernelGGL(k_eap_stress<decltype(LAST)::value>, gT, B2D, 0, c->stream, s, c->E, SB, c->p.arlx1i, c->p.denom1, hist);
        });
        hipLaunchKernelGGL(k_eap_stepu, gU, B2D, 0, c->stream, s, c->E, c->p, SB);
        if (ksub % 10 == 1) hipLaunchKernelGGL(k_eap_stepa, gT, B2D, 0, c->stream, s, c->E, SB, dtei);     // :411-426
        if (halo(c, SB + S_U, 2, true, true, 0.0)) return 1;                                               // :431-439
        c->bound_updates++;
        c->kernel_launches += 2;
        c->ksub++;
    }
    if (c->zone_mode) { c->zone_left = 0; c->inner_ok = true; }
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(&c->loop_ms, c->ev0, c->ev1));
    return xp_check(c);
}

// dev_strips: the counts k_strip_flags2 / k_compact_strips left in the page-locked h_counts (valid once the stream has passed the
// copies evpk_prep queued)
static void take_counts(evpk_ctx *c) {
    c->icellt = (long long)c->h_counts[0];
    c->icellu = (long long)c->h_counts[1];
    c->nstrips2 = (int)(c->h_counts[2] & 0xffffffffull);
    if (c->tuned_icellt == -2) c->tuned_icellt = c->icellt;
    c->counts_pending = false;
}

// ---- the timers of the subcycle loop (events owned by the context: kev, bev) --------------------------------------------------
// Kernel timing by HIP events on the stream the launches go to, in SPANS: one event in front of a run of consecutive
// launches of one kind (1 or 2 subcycles per launch) and one behind it, launches 3..8 of every 20 by default
// (EVPK_TIME_KERNELS=2: every launch a span of its own, 0: none).  A span's time / its launches is the per-launch time as the
// stream's timeline has it (launch gaps included, the ~4-8 us an event pair costs spread over six launches), so that
// launches x average never exceeds the loop time.  A span ends early when the kind or the stream changes and in front of any
// halo / fold / exchange work.
struct LoopTimer {
    evpk_ctx *c;
    bool span_open = false, bound_open = false;
    int span_kind = 0, span_n = 0, span_len = 6;
    hipStream_t span_stream = nullptr;
    int start(int nsub) {       // before the loop: an event pair for every launch of the call, no span recorded yet
        while (c->time_kernels && (int)c->kev.size() < 2 * nsub + 2) { hipEvent_t e; HIPCHK(c, hipEventCreate(&e)); c->kev.push_back(e); }
        c->kev_kind.clear(); c->kev_count.clear();
        c->nkev = 0;
        span_len = c->time_kernels == 2 ? 1 : 6;
        return 0;
    }
    int close() {       // end the open span, if any
        if (!span_open) return 0;
        span_open = false;
        const int rc = hipEventRecord(c->kev[2 * c->nkev + 1], span_stream) != hipSuccess;
        c->kev_kind.push_back(span_kind); c->kev_count.push_back(span_n);
        c->nkev++;
        if (rc) FAIL(c, "hipEventRecord failed");
        return 0;
    }
    int begin(hipStream_t st, int kind) {       // in front of a launch of `kind` subcycles on `st`
        if (span_open && (kind != span_kind || st != span_stream) && close()) return 1;
        if (span_open || !c->time_kernels) return 0;
        if (c->time_kernels == 1 && c->kernel_launches % 20 != 3) return 0;      // (an event pair stalls the queue for a few microseconds)
        if (2 * c->nkev + 2 > (int)c->kev.size()) return 0;
        span_open = true; span_kind = kind; span_n = 0; span_stream = st;
        if (hipEventRecord(c->kev[2 * c->nkev], st) != hipSuccess) FAIL(c, "hipEventRecord failed");
        return 0;
    }
    int end() {         // behind that launch
        if (!span_open) return 0;
        return (++span_n >= span_len) ? close() : 0;
    }
    // the same sampling for the halo / fold / ghost-zone updates (what the reference books under timer_bound): an event pair
    // on the stream the update runs on, every 5th update by default
    void bound_begin(hipStream_t st) {
        (void)close();
        bound_open = c->time_kernels == 2 || (c->time_kernels == 1 && c->bound_updates % 5 == 2);
        c->bound_updates++;
        if (!bound_open) return;
        while ((int)c->bev.size() < 2 * c->bound_timed + 2) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { bound_open = false; return; } c->bev.push_back(e); }
        (void)hipEventRecord(c->bev[2 * c->bound_timed], st);
    }
    void bound_end(hipStream_t st) {
        if (!bound_open) return;
        (void)hipEventRecord(c->bev[2 * c->bound_timed + 1], st);
        c->bound_timed++;
        bound_open = false;
    }
    // after the loop's last event has completed: the sampled times scaled to all updates / all launches of a kind
    int reduce() {
        if (c->bound_timed) {
            double sum = 0.0;
            for (int k = 0; k < c->bound_timed; k++) {
                float ms = 0.f;
                HIPCHK(c, hipEventElapsedTime(&ms, c->bev[2 * k], c->bev[2 * k + 1]));
                sum += ms;
            }
            c->bound_ms = (float)(sum / c->bound_timed * c->bound_updates);
        }
        if (c->time_kernels) {
            // per kind: time of its spans / launches inside them, scaled to all launches of that kind
            double sum[3] = {0, 0, 0};
            int cnt[3] = {0, 0, 0};
            for (int k = 0; k < c->nkev; k++) {
                float ms = 0.f;
                HIPCHK(c, hipEventElapsedTime(&ms, c->kev[2 * k], c->kev[2 * k + 1]));
                sum[c->kev_kind[k]] += ms; cnt[c->kev_kind[k]] += c->kev_count[k];
            }
            const int n1 = c->kernel_launches - c->double_launches;
            if (cnt[1]) c->kernel_ms = (float)(sum[1] / cnt[1] * n1);
            if (cnt[2]) c->kernel2_ms = (float)(sum[2] / cnt[2] * c->double_launches);
            c->kernel_timed = cnt[1]; c->kernel2_timed = cnt[2];
        }
        return 0;
    }
};

// ---- the subcycle loop: what its steps share during one call -------------------------------------------------------------------
struct SubLoop {
    evpk_ctx *c;
    LoopTimer t;
    int nsub, n = 0;            // subcycles of this call, of which done
    bool wrap, need_halo, revp;
    int G;                      // ghost-zone columns beyond the halo column the pair kernels compute (x-slabs)
    bool pendingI = false;      // an interior launch on stream2 that `stream` has not waited for yet
    bool evE_valid = false;     // evE marks the latest kernel launch on `stream`

    int join() {                // `stream` continues after the interior strips on stream2
        if (!pendingI) return 0;
        pendingI = false;
        if (hipStreamWaitEvent(c->stream, c->evI, 0) != hipSuccess) FAIL(c, "hipStreamWaitEvent failed");
        return 0;
    }
    // refresh the ghost zones of state buffer `SBUF` from the neighbours (it must hold the current state)
    // with_mirror (x-slab ranks on a tripole grid, another pair follows): the refresh of the mirror slab travels in the same round --
    // both exchanges are posted before either is waited for (peer-mapped: the mirror messages on the second channel, whose pages and
    // counters the zone messages do not touch; RCCL: one group), so that a pair of ranks meets once per refresh instead of twice
    int zone_exchange(int SBUF, bool with_mirror = false) {
        Slab &s = c->s;
        t.bound_begin(c->stream);
        if (with_mirror && c->xband && c->xb_merge && !c->relay) {
            XbXchg X;
            ColsXchg Q;
            const PairList pl = state_pairs(SBUF);
            if (xband_state(c, SBUF, c->stream, XP_POST, &X, c->ipc ? 1 : -1)) return 1;
            if (exchange_cols(c, pl, c->zcompact, XP_POST, &Q)) return 1;
            if (!c->ipc) NCCLCHK(c, ncclGroupStart());
            int rc = exchange_cols(c, pl, c->zcompact, XP_DONE, &Q);
            rc |= xband_state(c, SBUF, c->stream, XP_DONE, &X);
            if (!c->ipc && ncclGroupEnd() != ncclSuccess) FAIL(c, "zone + mirror exchange: ncclGroupEnd failed");
            if (rc) return 1;
            if (exchange_cols(c, pl, c->zcompact, XP_UNPACK, &Q)) return 1;
            if (xband_state(c, SBUF, c->stream, XP_UNPACK, &X)) return 1;
            c->xb_swaps++;
        } else {
            if (exchange_cols(c, state_pairs(SBUF), c->zcompact)) return 1;
            with_mirror = false;
        }
        t.bound_end(c->stream);
        c->zone_exchanges++;
        c->zone_bytes += (long long)(NSTATE / 2) * c->zW * 16 *
                         ((c->west >= 0 ? (c->zcompact ? c->zn[0] : s.nyl + 2) : 0) + (c->east >= 0 ? (c->zcompact ? c->zn[1] : s.nyl + 2) : 0));
        c->zone_left = c->zM;
        c->inner_ok = true;
        c->m_need = with_mirror ? 0 : 1;              // (x-slab tripole: the mirror slab is due as well)
        return 0;
    }
};

// EVPK_DEBUG_CLOCKS=<file>: the timeline of the loop's sixth launch (per strip: start / end clock of its wave, where it ran)
static int dbg_clocks_arm(evpk_ctx *c, SubArgs &a) {
    if (!(c->dbg_file && c->kernel_launches == 5 && c->evp_count == 3)) return 0;
    if (!c->d_dbg) { HIPCHK(c, hipMalloc(&c->d_dbg, sizeof(unsigned long long) * 4 * 65536)); }
    HIPCHK(c, hipMemsetAsync(c->d_dbg, 0, sizeof(unsigned long long) * 4 * 65536, c->stream));
    hipLaunchKernelGGL(k_dbg_clock, dim3(1), dim3(64), 0, c->stream, c->d_dbg + 4 * 65535);      // the stream's clock just before the launch
    a.dbg = c->d_dbg;
    return 0;
}

static int dbg_clocks_dump(evpk_ctx *c) {
    if (!(c->dbg_file && c->d_dbg && c->evp_count == 3)) return 0;
    std::vector<unsigned long long> h((size_t)4 * 65536);
    hipLaunchKernelGGL(k_dbg_clock, dim3(1), dim3(64), 0, c->stream, c->d_dbg + 4 * 65535 + 1);
    HIPCHK(c, hipMemcpy(h.data(), c->d_dbg, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
    if (FILE *fp = fopen(c->dbg_file, "w")) {
        fprintf(fp, "# t0 %llu\n", h[(size_t)4 * 65535]);
        for (int k = 0; k < 65535; k++) if (h[(size_t)4 * k]) fprintf(fp, "%d %llu %llu %llx\n", k, h[(size_t)4 * k], h[(size_t)4 * k + 1], h[(size_t)4 * k + 2]);
        fclose(fp);
    }
    return 0;
}

// ---- the tripole band of a pair: rows next to the fold are redone one subcycle at a time with the fold in between ------------------
//   band 1: T rows nyl-2..nyl+1, U rows nyl-2..nyl   state `sr` -> scratch;  fold(scratch)
//   band 2: T rows nyl-1..nyl+1, U rows nyl-1..nyl   scratch -> state `sw`;  fold(sw)
// The main launch leaves rows >= nyl-1 to the bands (jmax).  Three ways, each fills in its part of the main launch's arguments:

// tripole on ONE rank: the top band of a pair runs as extra workgroups of the pair's own launch (band_pair: a strip
// and its mirror image in one workgroup, the fold between the subcycles in its LDS) -- no band launches, no second
// stream, no hand-overs; EVPK_BAND_FUSED=0 brings the launches on stream2 back
static void band_fused(const SubLoop &L, SubArgs &a) {
    const Slab &s = L.c->s;
    a.nband = (s.nxl / 2 + 1 + 60) / 61;          // strips A cover columns 0 .. nx/2, their mirror images the rest
    a.jmax = s.nyl - 2;
}

// x-slab ranks: strip A of every band workgroup is mine, strip B the mirror rank's, read from the mirror slab M.
// M comes whole after a ghost-zone exchange or a one-subcycle launch (one message, m_need); between two such
// refreshes its rows below the band are advanced HERE by the pair kernel over M's own strips (two rows of
// validity less per pair, see evpk_connect) and the band rows by band_pair, on both ranks alike
static int band_xslab(SubLoop &L, SubArgs &a, bool pair_ends_evp) {
    evpk_ctx *c = L.c;
    Slab &s = c->s;
    if (L.join()) return 1;
    if (c->m_need) {
        L.t.bound_begin(c->stream);
        if (xband_state(c, a.sr, c->stream)) return 1;
        L.t.bound_end(c->stream);
        c->xb_swaps++;
        c->m_need = 0;
    }
    // (cells no lane stores are alike in both state buffers: M's write buffer starts from its read buffer)
    hipLaunchKernelGGL(k_xband_rows_copy, dim3((s.nxl + 2 * ZW_MAX + 127) / 128, c->m.nyl + 2), dim3(128), 0, c->stream, c->m, a.sr, a.sw,
                       (int)NSTATE, 0, c->m.nyl + 1);
    if (c->zone_left > 1 && !pair_ends_evp) {      // another pair follows before the next refresh
        if (c->ms_R != c->R2 || c->ms_ncx != c->ncx2) {
            const int nry = (c->m.nyl + c->R2 - 1) / c->R2;
            std::vector<int> ms((size_t)c->ncx2 * nry);
            for (int k = 0; k < (int)ms.size(); k++) ms[k] = k;
            if (c->d_mstrips) (void)hipFree(c->d_mstrips);
            c->d_mstrips = nullptr;
            HIPCHK(c, hipMalloc(&c->d_mstrips, sizeof(int) * ms.size()));
            HIPCHK(c, hipMemcpy(c->d_mstrips, ms.data(), sizeof(int) * ms.size(), hipMemcpyHostToDevice));
            c->ms_R = c->R2; c->ms_ncx = c->ncx2; c->ms_n = (int)ms.size();
        }
        SubArgs bm = a;
        bm.s = c->m; bm.strips = c->d_mstrips; bm.nstrips = c->ms_n; bm.nsdev = nullptr; bm.jmax = c->m.nyl - 2;
        // M's advance writes M's rows below the band, the band workgroups of the main launch the rows above, both read
        // the other state buffer: the advance runs as workgroups OF the main launch (SubArgs::nmir) -- a launch of its
        // own, seven to nine rows of dependent marching, took as long as the main launch of a narrow slab and sat in
        // front of every pair (round 4, xp_compare: 52 us per pair; on stream2 beside the main launch the two event
        // hand-overs cost more than that: 29.5 against 24.4 ms per evp, rejected).  EVPK_XB_FUSE=0: the launch of its own
        if (c->xb_fuse) { a.nmir = c->ms_n; a.mjmax = c->m.nyl - 2; }
        else launch_sub2(c, bm, c->stream, L.revp, false);
    }
    a.xm = c->d_mslab;
    a.nband = (s.nxl + 2 * L.G + 60) / 61;
    a.jmax = s.nyl - 2;
    return 0;
}

// band launches (k_subcycle_t) on stream2, beside the main launch: nothing the band sequence -- band 1, fold, band 2,
// fold -- reads or writes is touched by it (single rank: the main launch writes its own E-W ghost images;
// x-slabs: those come with the ghost-zone exchange after both).  `stream` takes over again after the main launch (step_pair).
static int band_stream2(SubLoop &L, SubArgs &a, bool pair_ends_evp) {
    evpk_ctx *c = L.c;
    Slab &s = c->s;
    SubArgs b1 = a;
    b1.strips = c->d_band; b1.nstrips = c->ncx; b1.ncx = c->ncx; b1.wrap = L.wrap ? 1 : 0; b1.G = 0;
    b1.R = 4; b1.jb0 = s.nyl - 2; b1.sw = F_STATE2;
    SubArgs b2 = b1;
    b2.R = 3; b2.jb0 = s.nyl - 1; b2.sr = F_STATE2; b2.sw = a.sw;
    if (c->handover_value) {
        c->sig_seq++;
        HIPCHK(c, hipStreamWriteValue32(c->stream, c->sigB, c->sig_seq, 0));
        HIPCHK(c, hipStreamWaitValue32(c->stream2, c->sigB, c->sig_seq, hipStreamWaitValueGte, 0xFFFFFFFFu));
    } else {
        HIPCHK(c, hipEventRecord(c->evB0, c->stream));          // the previous pair (and its exchange) is complete
        HIPCHK(c, hipStreamWaitEvent(c->stream2, c->evB0, 0));
    }
    launch_sub1t(b1, c->stream2, L.revp, false);
    L.t.bound_begin(c->stream2);
    if (halo(c, F_STATE2 + S_U, 2, true, true, 0.0, -1, c->stream2, false, a.sr + S_U)) return 1;
    L.t.bound_end(c->stream2);
    launch_sub1t(b2, c->stream2, L.revp, pair_ends_evp);
    L.t.bound_begin(c->stream2);
    // (x-slabs: the ghost-zone exchange after the pair delivers the E-W ghost columns of the new state, all rows)
    if (halo(c, a.sw + S_U, 2, true, true, 0.0, -1, c->stream2, c->zone_mode, F_STATE2 + S_U, s.nyl - 1)) return 1;
    L.t.bound_end(c->stream2);
    if (c->handover_value) HIPCHK(c, hipStreamWriteValue32(c->stream2, c->sigB1, c->sig_seq, 0));
    else HIPCHK(c, hipEventRecord(c->evB1, c->stream2));
    a.jmax = s.nyl - 2;
    return 0;
}

// the main launch of a pair.  split (x-slabs): the launch that uses up the zones runs its edge strips first on `stream`, followed by
// the exchange of the edge columns there, while the interior strips run on `stream2`
static int pair_launch(SubLoop &L, SubArgs &a, bool split, bool pair_ends_evp) {
    evpk_ctx *c = L.c;
    if (L.join()) return 1;
    if (!split) {
        if (c->nstrips2 > 0) {
            if (L.t.begin(c->stream, 2)) return 1;
            launch_sub2(c, a, c->stream, L.revp, pair_ends_evp);
            if (L.t.end()) return 1;
            c->kernel_launches++;
            c->double_launches++;
        }
        L.evE_valid = false;
        return 0;
    }
    // edge(k) reads everything round k-1 wrote near the edges: interior(k-1) on stream2 (joined above), the exchange on stream
    if (!L.evE_valid) HIPCHK(c, hipEventRecord(c->evE, c->stream));      // round k-1 was a plain launch on `stream`
    a.strips = c->d_strips2e; a.nstrips = c->nstrips2e;
    launch_sub2(c, a, c->stream, L.revp, false);
    // interior(k) needs round k-1's kernels, not its exchange: it reads no ghost zone
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->evE, 0));
    a.strips = c->d_strips2i; a.nstrips = c->nstrips2i;
    if (L.t.begin(c->stream2, 2)) return 1;
    launch_sub2(c, a, c->stream2, L.revp, false);
    if (L.t.end()) return 1;
    if (L.t.close()) return 1;      // (the other stream's work follows)
    c->kernel_launches++;
    c->double_launches++;
    HIPCHK(c, hipEventRecord(c->evI, c->stream2));
    L.pendingI = true;
    HIPCHK(c, hipEventRecord(c->evE, c->stream));
    L.evE_valid = true;
    return 0;
}

// two subcycles in one launch; pair_ends_evp: the second is the last of this evp (else another subcycle follows it: "pair_inside")
static int step_pair(SubLoop &L, SubArgs &a, bool fused_band, bool xb, bool pair_ends_evp) {
    evpk_ctx *c = L.c;
    a.strips = c->d_strips2; a.nstrips = c->dev_strips ? c->ns_tot2_cur : c->nstrips2; a.ncx = c->ncx2; a.R = c->R2; a.G = L.G;
    a.nsdev = c->dev_strips ? c->d_ns2 : nullptr;
    a.wrap = (c->ew == EVPK_BND_CYCLIC && !c->zone_mode) ? 1 : 0;      // in-kernel cyclic wrap, or ghost-zone mode
    if (c->zone_mode && c->zone_left < 1) {         // (a one-subcycle launch or a partial call came before)
        if (L.join()) return 1;
        if (L.zone_exchange(a.sr)) return 1;
    }
    const bool band2 = c->band_mode && !fused_band && !xb;
    if (fused_band) band_fused(L, a);
    else if (xb) { if (band_xslab(L, a, pair_ends_evp)) return 1; }
    else if (band2) { if (band_stream2(L, a, pair_ends_evp)) return 1; }
    const bool split = c->zone_mode && c->overlap && !c->band_mode && !pair_ends_evp && c->zone_left == 1 &&
                       c->nstrips2e > 0 && c->nstrips2i > 0;
    if (pair_launch(L, a, split, pair_ends_evp)) return 1;
    if (band2 && c->handover_value) HIPCHK(c, hipStreamWaitValue32(c->stream, c->sigB1, c->sig_seq, hipStreamWaitValueGte, 0xFFFFFFFFu));
    else if (band2) HIPCHK(c, hipStreamWaitEvent(c->stream, c->evB1, 0));
    c->ksub += 2;
    L.n += 2;
    c->cur ^= 1;
    if (c->zone_mode) {
        c->zone_left--;
        c->inner_ok = c->zone_left >= 1;
        // the zones are used up (in a split round this overlaps the interior strips), or the evp is complete
        if (c->zone_left < 1 || pair_ends_evp) {
            if (!split && L.join()) return 1;
            if (L.zone_exchange(c->cur ? F_STATE1 : F_STATE0, !pair_ends_evp && L.nsub - L.n >= 2 && c->p.ndte - c->ksub >= 2)) return 1;
        }
    }
    return 0;
}

// one subcycle: eap (stress_eap + stepu in one launch), one row per wave on a small slab, else marching; then the velocity halo
static int step_single(SubLoop &L, SubArgs &a) {
    evpk_ctx *c = L.c;
    Slab &s = c->s;
    if (L.join()) return 1;
    if (c->zone_mode && !c->inner_ok && L.zone_exchange(a.sr)) return 1;
    if (strips1(c)) return 1;
    c->ksub++;
    L.n++;
    a.strips = c->d_strips; a.nstrips = c->nstrips; a.ncx = c->ncx; a.wrap = L.wrap ? 1 : 0;
    a.R = c->R;                     // (strips1 may have re-tuned it: tune_R1)
    const bool last = (c->ksub == c->p.ndte);
    if (c->nstrips > 0) {
        // small slab: one row per wave (k_subcycle_t) instead of R + 1 march steps per wave
        const bool t1 = c->R <= 7 && (long long)c->nstrips * (c->R + 1) <= 8LL * c->nsimd && c->tile_force != 0;
        if (L.t.begin(c->stream, 1)) return 1;
        if (c->eap) {       // eap(dt): stress_eap + stepu in one launch (k_eap_sub), stepa every tenth subcycle (ice_dyn_eap.F90:345-447)
            EapSubArgs x{c->E, (last || L.n == L.nsub) ? 1 : 0};
            with_bool(last, [&](auto LAST) {
                hipLaunchKernelGGL(k_eap_sub<decltype(LAST)::value>, dim3(xcd_round((c->nstrips + 3) / 4)), dim3(256), 0, c->stream, a, x);
            });
            // (round 5: stepa INSIDE this launch -- the angle planes double buffered, the twelve stepa subcycles as a kernel of their own
            //  at three waves per SIMD -- was built, is bit-exact and measured SLOWER: 42.1-43.0 ms per eap against 41.2-41.3,
            //  profiles/r05_v1/eap_stepa_ab.txt; the launch of its own stays)
            if (c->ksub % 10 == 1) {                                                    // :411-426
                const double dtei = 1.0 / (c->p.dt / (double)c->p.ndte);              // ice_dyn_shared.F90:209-210
                hipLaunchKernelGGL(k_eap_stepa, dim3((s.nxl + 1 + 63) / 64, (s.nyl + 1 + 3) / 4), B2D, 0, c->stream, s, c->E, a.sw, dtei);
            }
        }
        else if (t1) launch_sub1t(a, c->stream, L.revp, last);
        else launch_sub1(a, c->stream, L.revp, last);
        if (L.t.end()) return 1;
        c->kernel_launches++;
    }
    L.evE_valid = false;
    c->cur ^= 1;
    if (L.need_halo) {                                                          // ice_dyn_evp.F90:392-400
        L.t.bound_begin(c->stream);
        if (halo(c, (c->cur ? F_STATE1 : F_STATE0) + S_U, 2, true, true, 0.0, -1, nullptr, false, a.sr + S_U)) return 1;
        L.t.bound_end(c->stream);
    }
    if (c->zone_mode) { c->zone_left = 0; c->inner_ok = true; }     // one ghost column is current, the deeper zone is not
    c->m_need = 1;
    return 0;
}

static int subcycle_impl(evpk_ctx *c, int32_t nsub) {
    if (!c->prepped) FAIL(c, "evpk_prep has not been called");
    if (nsub < 0) FAIL(c, "nsub < 0");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->eap) {       // EVPK_EAP_FUSED=0: stress_eap and stepu as two launches with str(8) through memory, in place
        const char *e = getenv("EVPK_EAP_FUSED");
        if (e && atoi(e) == 0) return eap_subcycle(c, nsub);
    }
    SubLoop L{c, LoopTimer{c}, nsub};
    L.wrap = (c->nranks == 1 && c->ew == EVPK_BND_CYCLIC && !c->force_exchange);
    L.need_halo = (c->nranks > 1) || (c->ns == EVPK_BND_TRIPOLE) || c->force_exchange;
    L.revp = (c->p.revp == 1.0);
    L.G = c->zone_mode ? c->zW - 2 : 0;
    reset_call_counters(c);
    if (L.t.start(nsub)) return 1;
    const bool ov_trying = c->zone_mode && !c->band_mode && !c->ov_fixed && c->ksub == 0 && nsub == c->p.ndte;
    if (ov_trying) c->overlap = (c->ov_trial != 2);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (c->eap && c->ksub == 0) hipLaunchKernelGGL(k_eap_reset, grid2d(s, B2D), B2D, 0, c->stream, s, c->E);   // ice_dyn_eap.F90:171-180, :284-298
    while (L.n < nsub) {
        SubArgs a;
        a.s = s; a.ecci = c->p.ecci; a.arlx1i = c->p.arlx1i; a.denom1 = c->p.denom1; a.brlx = c->p.brlx;
        a.revp = c->p.revp; a.cosw = c->p.cosw; a.sinw = c->p.sinw;
        a.R = c->R; a.jb0 = 0; a.G = 0; a.jmax = 1 << 30; a.nband = 0; a.nmir = 0; a.mjmax = 0; a.nsdev = nullptr; a.xm = nullptr; a.dbg = nullptr; a.prio = c->prio; a.band_last = c->band_last;      // (band_last: switched off in launch_sub2 for the tile kernels)
        a.sr = c->cur ? F_STATE1 : F_STATE0; a.sw = c->cur ? F_STATE0 : F_STATE1;
        const int left = nsub - L.n;
        // two subcycles in one launch when neither of them is the last one of this evp (ksub == ndte writes diagnostics) ...
        // (a small slab on a one-rank tripole grid: the band sequence of a pair -- two band launches, two folds, two hand-overs
        // between the streams, ~35 us -- costs more than two one-row-per-wave launches with their folds on one stream: 2.4 ms
        // against 1.9 per evp at 360x300, even at 720x540, measured again with the stream-memory hand-overs)
        const bool fused_band = c->band_mode && c->band_fused && L.wrap && s.nyl >= 4;      // see band_fused
        const bool xb = c->xband && !fused_band;
        const bool pairs = c->use_double && !c->eap && (fused_band || !(c->band_mode && c->tile_mode && c->nranks == 1 && !c->force_exchange));
        const bool pair_inside = pairs && left >= 2 && c->ksub + 2 < c->p.ndte;
        // ... or when the second of them is the last one (the pair kernels' LAST2 variants; tripole: the second band launch is then
        // the LAST variant of k_subcycle)
        const bool pair_ends_evp = pairs && left >= 2 && (c->ksub + 2 == c->p.ndte);
        if (dbg_clocks_arm(c, a)) return 1;
        if (pair_inside || pair_ends_evp) { if (step_pair(L, a, fused_band, xb, pair_ends_evp)) return 1; }
        else if (step_single(L, a)) return 1;
    }
    if (L.t.close()) return 1;
    if (L.join()) return 1;
    // leave the ghost columns 0 / nxl+1 of the state current (download, finish, a later one-subcycle launch)
    if (c->zone_mode && !c->inner_ok && L.zone_exchange(c->cur ? F_STATE1 : F_STATE0)) return 1;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventSynchronize(c->ev1));
    HIPCHK(c, hipEventElapsedTime(&c->loop_ms, c->ev0, c->ev1));
    if (dbg_clocks_dump(c)) return 1;
    if (c->dev_strips) take_counts(c);   // what evpk_prep left in flight has arrived with the loop's last event
    if (xp_check(c)) return 1;
    if (ov_trying) {
        if (c->ov_trial >= 1) c->ov_ms[c->ov_trial - 1] = c->loop_ms;
        if (++c->ov_trial == 3) { c->overlap = (c->ov_ms[0] <= c->ov_ms[1]); c->ov_fixed = true; }
    }
    return L.t.reduce();
}

extern "C" int evpk_subcycle(evpk_ctx *c, int32_t nsub) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c) return 1;
    const int rc = subcycle_impl(c, nsub);
    if (rc) {   // an error return must not leave work or event waits outstanding on either stream
        if (c->stream2) (void)hipStreamSynchronize(c->stream2);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
    }
    return rc;
}

extern "C" int evpk_finish(evpk_ctx *c) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c) return 1;
    if (!c->prepped) FAIL(c, "evpk_prep has not been called");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const dim3 g2 = grid2d(s, B2D);
    const int SB = c->cur ? F_STATE1 : F_STATE0;
    if (c->ns == EVPK_BND_TRIPOLE && !c->eap && halo_stress12(c, SB + S_SP)) return 1;        // ice_dyn_evp.F90:454-479 (eap has none)
    if (c->nranks == 1 && !c->force_exchange && c->finish_fused) {
        // one rank: evp_finish and u2tgrid_vector in one launch, the ghost values of the work pair computed where they are read
        hipLaunchKernelGGL(k_finish_tgrid, g2, B2D, 0, c->stream, s, c->p, c->cur, c->ew == EVPK_BND_CYCLIC ? 1 : 0, c->ns == EVPK_BND_TRIPOLE ? 1 : 0);
    } else {
        hipLaunchKernelGGL(k_finish, g2, B2D, 0, c->stream, s, c->p, c->cur);        // :487-503
        // u2tgrid_vector (:505-506, ice_grid.F90:1886-1910)
        if (halo(c, F_WORK3, 2, true, true, 0.0)) return 1;
        hipLaunchKernelGGL(k_to_tgrid2, g2, B2D, 0, c->stream, s);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int evpk_sync(evpk_ctx *c) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int evpk_download(evpk_ctx *c, evpk_state *st) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !st) return 1;
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const int SB = c->cur ? F_STATE1 : F_STATE0;
    // sparse transfers: tiles that are inactive now and were at the previous evp hold the same zeros on both sides (s.act_any)
    // ... which is only known of an array that was also delivered after the previous evp: one that the caller fetches now
    // and then (restart, history) is delivered whole
    const unsigned char *act_all = (c->io_sparse_now && c->prepped) ? s.act_any : nullptr;
    XferBatch DB;
    DB.c = c; DB.up = false;
    const size_t nall = (size_t)c->nblocks * c->nyb * c->nxb;
    auto dl = [&](double *h, int f, int mode, int id, bool never_sparse = false) -> int {
        if (!h || !c->nblocks) return 0;
        const unsigned char *a = (!never_sparse && act_all && c->last_dl[id] == c->evp_count - 1) ? act_all : nullptr;
        c->last_dl[id] = c->evp_count;
        double *dst = (c->xfer_fused && !c->verify_delivery) ? (double *)mapped_alias(h, nall * sizeof(double)) : nullptr;
        if (!dst) return download_f(c, h, f, mode, a);
        if (DB.L.n && (DB.act != a || DB.L.n == XFER_MAX)) { if (DB.flush()) return 1; }
        DB.act = a;
        DB.L.f[DB.L.n] = f; DB.L.mode[DB.L.n] = mode; DB.L.host[DB.L.n] = dst; DB.L.n++;
        return 0;
    };
    if (dl(st->uvel, SB + S_U, MODE_ALL, F_STATE0 + S_U)) return 1;
    if (dl(st->vvel, SB + S_V, MODE_ALL, F_STATE0 + S_V)) return 1;
    const int smode = (c->ns == EVPK_BND_TRIPOLE) ? MODE_NE_FOLD : MODE_NE;
    for (int q = 0; q < 4; q++) {
        if (dl(st->stressp[q], SB + S_SP + q, smode, F_STATE0 + S_SP + q)) return 1;
        if (dl(st->stressm[q], SB + S_SM + q, smode, F_STATE0 + S_SM + q)) return 1;
        if (dl(st->stress12[q], SB + S_S12 + q, smode, F_STATE0 + S_S12 + q)) return 1;
    }
    if (download_m(c, st->iceumask, s.iceumask, MODE_PHYS)) return 1;
    struct { double *h; int f; } op[] = {
        {st->divu, F_DIVU}, {st->shear, F_SHEAR}, {st->rdg_conv, F_RDGCONV}, {st->rdg_shear, F_RDGSHEAR},
        {st->prs_sig, F_PRSSIG}, {st->strintx, F_STRINTX}, {st->strinty, F_STRINTY}, {st->strocnx, F_STROCNX},
        {st->strocny, F_STROCNY}, {st->strocnxT, F_STROCNXT}, {st->strocnyT, F_STROCNYT}, {st->strairx, F_STRAIRX},
        {st->strairy, F_STRAIRY}, {st->strtltx, F_STRTLTX}, {st->strtlty, F_STRTLTY}, {st->fm, F_FM},
        {st->tmass, F_TMASS}, {st->aiu, F_AIU}, {st->umass, F_UMASS}, {st->uvel_init, F_UVEL_INIT}, {st->vvel_init, F_VVEL_INIT}};
    for (auto &e : op) {
        // strairx/y after t2ugrid_vector: to_ugrid zeroes the whole array before it fills the physical cells (ice_grid.F90:1852)
        const bool zg = (e.f == F_STRAIRX || e.f == F_STRAIRY) && !c->p.wind_on_ugrid;
        if (dl(e.h, e.f, zg ? MODE_PHYS_ZG : MODE_PHYS, e.f, zg)) return 1;
    }
    if (DB.flush()) return 1;
    // the strength with its ghost cells halo-updated, as evp leaves it (ice_dyn_evp.F90:311-312) -- also when it was an input
    if (download_f(c, st->strength, F_STRENGTH, MODE_ALL)) return 1;
    if (st->icetmask) {
        // icetmask travels as a 0/1 double plane on the device; convert through the staging buffer
        std::vector<double> tmp((size_t)c->nblocks * c->nyb * c->nxb, 0.0);
        if (download_f(c, tmp.data(), F_ICETM, MODE_ALL)) return 1;
        for (size_t k = 0; k < tmp.size(); k++) st->icetmask[k] = (int32_t)tmp[k];
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // scatter kernels into page-locked host arrays
    return xp_check(c);
}

extern "C" int evpk_run(evpk_ctx *c, const evpk_step_in *in, evpk_state *st) {
    if (!c) return 1;
    if (evpk_upload(c, in, st)) return 1;
    if (evpk_prep(c)) return 1;
    if (evpk_subcycle(c, c->p.ndte)) return 1;
    if (evpk_finish(c)) return 1;
    return evpk_download(c, st);
}

extern "C" int evpk_principal_stress(evpk_ctx *c, double *sig1, double *sig2) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !sig1 || !sig2) return 1;
    if (!c->prepped) FAIL(c, "evpk_principal_stress needs the state of a finished evp on the device");
    HIPCHK(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_principal_stress, grid2d(c->s, B2D), B2D, 0, c->stream, c->s, c->cur ? (int)F_STATE1 : (int)F_STATE0);
    HIPCHK(c, hipGetLastError());
    if (download_f(c, sig1, F_SIG1, MODE_PHYS) || download_f(c, sig2, F_SIG2, MODE_PHYS)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- ice_HaloUpdate / ice_HaloUpdate_stress of a caller's block array on the device (SURVEY S8 row a3 as an entry point) ----
// planes of the caller's block arrays (p: the plane of block 0, bstride: doubles from block to block) through the scratch state planes
// and the general update, max_nf planes at a time; field_loc / field_type as evpk_halo_update's
struct BlockPlane { double *p; size_t bstride; };
static int block_planes_halo(evpk_ctx *c, const std::vector<BlockPlane> &pl, int field_loc, int field_type, double fill) {
    Slab &s = c->s;
    const dim3 b(64), g = block_grid(c);
    const bool necorner = (field_loc == 2), vector = (field_type != 1);
    const int loc_x = field_loc == 4 ? 2 : field_loc == 3 ? 3 : -1;            // k_fold_apply's codes for E face / N face
    const int chunk = std::min(c->max_nf, (int)NSTATE), np = (int)pl.size();
    for (int k0 = 0; k0 < np; k0 += chunk) {
        const int nf = std::min(chunk, np - k0);
        for (int q = 0; q < nf; q++) {
            if (!c->full_cover) hipLaunchKernelGGL(k_fill_plane, grid2d(s, B2D), B2D, 0, c->stream, s, (int)F_STATE2 + q, fill);
            LAUNCH_BLOCKS(k_gather_fs, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)pl[k0 + q].p, pl[k0 + q].bstride, (int)F_STATE2 + q);
        }
        if (halo(c, F_STATE2, nf, necorner, vector, fill, -1, nullptr, false, -1, 0, loc_x)) return 1;
        for (int q = 0; q < nf; q++)
            LAUNCH_BLOCKS(k_scatter_halo, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (int)F_STATE2 + q, pl[k0 + q].p, pl[k0 + q].bstride, fill,
                          c->ew == EVPK_BND_CYCLIC ? 1 : 0, c->ns == EVPK_BND_TRIPOLE ? 1 : 0, (field_loc == 2 || field_loc == 3) ? 1 : 0, 0, -1);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// which ghost cells border an eliminated land block: the coverage of the slab in plane f, halo-updated like any centre scalar (1 beyond an
// open / closed boundary: no neighbour at all).  fcov = f, or -1 where no block is missing and the plane is not written
static int cover_plane(evpk_ctx *c, int f, int &fcov) {
    fcov = -1;
    if (c->full_cover && c->nranks == 1) return 0;     // (collective: another rank may have an eliminated block where this one has none)
    hipLaunchKernelGGL(k_fill_plane, grid2d(c->s, B2D), B2D, 0, c->stream, c->s, f, 0.0);
    LAUNCH_BLOCKS(k_cover_f, block_grid(c), dim3(64), 0, c->stream, c->s, c->d_bd, c->nxb, c->nyb, f);
    if (halo(c, f, 1, false, false, 1.0)) return 1;
    fcov = f;
    return 0;
}

extern "C" int evpk_halo_update(evpk_ctx *c, double *a, int32_t nz, int32_t field_loc, int32_t field_type, double fill) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !a) return 1;
    if (!c->connected) FAIL(c, "evpk_halo_update: the context is not connected yet (evpk_connect)");
    if (nz < 0 || field_loc < 1 || field_loc > 4 || field_type < 1 || field_type > 3) FAIL(c, "evpk_halo_update: bad nz / field_loc / field_type");
    HIPCHK(c, hipSetDevice(c->device));
    const int np = nz > 0 ? nz : 1;
    const size_t nblk = (size_t)c->nyb * c->nxb, n = (size_t)c->nblocks * np * nblk;
    double *dev = nullptr;
    std::vector<HostArr> arr = {{a, n, &dev, true}};
    if (stage_in(c, arr)) return 1;
    std::vector<BlockPlane> pl;
    for (int k = 0; k < np; k++) pl.push_back({dev + (size_t)k * nblk, (size_t)np * nblk});
    if (block_planes_halo(c, pl, field_loc, field_type, fill)) return 1;
    if (stage_out(c, arr)) return 1;
    return xp_check(c);
}

extern "C" int evpk_halo_update_stress(evpk_ctx *c, double *a1, const double *a2) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !a1 || !a2) return 1;
    if (!c->connected) FAIL(c, "evpk_halo_update_stress: the context is not connected yet (evpk_connect)");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nblk = (size_t)c->nyb * c->nxb, n = (size_t)c->nblocks * nblk;
    double *d1 = nullptr;
    const double *d2 = nullptr;
    std::vector<HostArr> arr = {{a1, n, &d1, true}, {a2, n, &d2, false}};
    if (stage_in(c, arr)) return 1;
    const dim3 b(64), g = block_grid(c);
    const int fA = F_STATE2, fB = F_STATE2 + 1, fC = F_STATE2 + 2;
    int fcov;
    if (cover_plane(c, fC, fcov)) return 1;
    if (fcov >= 0) {
        hipLaunchKernelGGL(k_fill_plane, grid2d(s, B2D), B2D, 0, c->stream, s, fA, 0.0);
        hipLaunchKernelGGL(k_fill_plane, grid2d(s, B2D), B2D, 0, c->stream, s, fB, 0.0);
    }
    LAUNCH_BLOCKS(k_gather_fs, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)d1, nblk, fA);
    LAUNCH_BLOCKS(k_gather_fs, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, d2, nblk, fB);
    if (c->ns == EVPK_BND_TRIPOLE && halo(c, fA, 1, false, false, 0.0, fB)) return 1;
    LAUNCH_BLOCKS(k_scatter_halo, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, fA, d1, nblk, 0.0, c->ew == EVPK_BND_CYCLIC ? 1 : 0,
                       c->ns == EVPK_BND_TRIPOLE ? 1 : 0, 0, 1, fcov);
    HIPCHK(c, hipGetLastError());
    if (stage_out(c, arr)) return 1;
    return xp_check(c);
}

// ---- the dynamics records of the binary restart (source/ice_restart_driver.F90:122-176 dumpfile, :295-412 restartfile) ---------
// uvel, vvel, strocnxT, strocnyT, the twelve stresses in the order 1,3,2,4 ("read and scattered in pairs in order to properly
// match corner values across a tripole grid cut", :343-345) and iceumask as real 0/1: one Fortran sequential unformatted
// record each (4-byte length, the (nx_global, ny_global) real*8 array as the master task holds it after gather_global,
// 4-byte length; io_binary/ice_restart.F90:641-684 -> ice_write 'ruf8'), big-endian under the production flags
// (bld/Macros.nci: -convert big_endian).  Straight from / into the state resident on the device.
static const int kRestartOrder[4] = {0, 2, 1, 3};      // sigma_1, sigma_3, sigma_2, sigma_4

static void swap8(double *a, size_t n) {
    for (size_t k = 0; k < n; k++) {
        uint64_t v; memcpy(&v, &a[k], 8);
        v = __builtin_bswap64(v);
        memcpy(&a[k], &v, 8);
    }
}

static std::vector<int> restart_fields(const evpk_ctx *c) {
    const int SB = c->cur ? F_STATE1 : F_STATE0;
    std::vector<int> f = {SB + S_U, SB + S_V, F_STROCNXT, F_STROCNYT};
    for (int fam : {S_SP, S_SM, S_S12}) for (int q = 0; q < 4; q++) f.push_back(SB + fam + kRestartOrder[q]);
    f.push_back(-1);                                   // iceumask
    return f;
}

extern "C" int evpk_restart_write(evpk_ctx *c, const char *path, int32_t append, int32_t big_endian) {
    if (!c || !path) return 1;
    if (!c->uploaded) FAIL(c, "evpk_restart_write: no state on the device");
    if (c->nranks != 1) FAIL(c, "evpk_restart_write: one rank only (the reference gathers to the master task, ice_gather_scatter.F90; download and use the host path)");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)s.nxg * s.nyg;
    if (n * 8 > 0x7fffffffu) FAIL(c, "evpk_restart_write: record longer than a 4-byte length marker holds");
    double *dG = nullptr;
    HIPCHK(c, hipMalloc(&dG, n * 8));
    std::vector<double> h(n);
    FILE *fp = fopen(path, append ? "ab" : "wb");
    if (!fp) { (void)hipFree(dG); FAIL(c, "evpk_restart_write: cannot open %s", path); }
    int rc = 0;
    for (int f : restart_fields(c)) {
        (void)hipMemsetAsync(dG, 0, n * 8, c->stream);                     // cells of eliminated land blocks: 0
        hipLaunchKernelGGL(k_slab_to_global, dim3((s.nxl + 127) / 128, s.nyl), dim3(128), 0, c->stream, s, f, dG);
        if (hipMemcpyAsync(h.data(), dG, n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { rc = 1; break; }
        uint32_t mark = (uint32_t)(n * 8);
        if (big_endian) { swap8(h.data(), n); mark = __builtin_bswap32(mark); }
        if (fwrite(&mark, 4, 1, fp) != 1 || fwrite(h.data(), 8, n, fp) != n || fwrite(&mark, 4, 1, fp) != 1) { rc = 2; break; }
    }
    fclose(fp);
    (void)hipFree(dG);
    if (rc) FAIL(c, "evpk_restart_write: %s", rc == 1 ? "device copy failed" : "write failed");
    return 0;
}

extern "C" int evpk_restart_read(evpk_ctx *c, const char *path, int64_t byte_offset, int32_t big_endian) {
    if (!c || !path) return 1;
    if (!c->connected) FAIL(c, "evpk_connect has not been called");
    if (c->nranks != 1) FAIL(c, "evpk_restart_read: one rank only (read on the host and upload)");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)s.nxg * s.nyg;
    double *dG = nullptr;
    HIPCHK(c, hipMalloc(&dG, n * 8));
    std::vector<double> h(n);
    FILE *fp = fopen(path, "rb");
    if (!fp) { (void)hipFree(dG); FAIL(c, "evpk_restart_read: cannot open %s", path); }
    if (byte_offset > 0 && fseek(fp, (long)byte_offset, SEEK_SET) != 0) { fclose(fp); (void)hipFree(dG); FAIL(c, "evpk_restart_read: bad offset"); }
    c->cur = 0;                                        // the state is read into buffer 0, as evpk_upload leaves it
    int rc = 0;
    for (int f : restart_fields(c)) {
        uint32_t m0 = 0, m1 = 0;
        if (fread(&m0, 4, 1, fp) != 1 || fread(h.data(), 8, n, fp) != n || fread(&m1, 4, 1, fp) != 1) { rc = 2; break; }
        if (big_endian) { m0 = __builtin_bswap32(m0); m1 = __builtin_bswap32(m1); swap8(h.data(), n); }
        if (m0 != (uint32_t)(n * 8) || m1 != m0) { rc = 3; break; }
        if (hipMemcpyAsync(dG, h.data(), n * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = 1; break; }
        hipLaunchKernelGGL(k_global_to_slab, dim3((s.nxl + 127) / 128, s.nyl), dim3(128), 0, c->stream, s, f, (const double *)dG);
        if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = 1; break; }
    }
    fclose(fp);
    (void)hipFree(dG);
    if (rc) FAIL(c, "evpk_restart_read: %s", rc == 1 ? "device copy failed" : rc == 2 ? "short read" : "record length marker does not match the grid (size / byte order?)");
    // ghost cells as restartfile leaves them: scatter_global's halo fill by field location / type (u, v: NE corner vectors,
    // :306-309; strocnxT/yT: centre vectors; stresses: centre scalars), then on tripole grids the twelve
    // ice_HaloUpdate_stress calls that pair the corners across the cut (:370-395)
    if (halo(c, F_STATE0 + S_U, 2, true, true, 0.0)) return 1;
    if (halo(c, F_STROCNXT, 2, false, true, 0.0)) return 1;
    if (halo(c, F_STATE0 + S_SP, 12, false, false, 0.0)) return 1;
    if (c->ns == EVPK_BND_TRIPOLE && halo_stress12(c, F_STATE0 + S_SP)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->uploaded = true;
    c->prepped = false;
    c->fresh = true;
    return 0;
}

// ---- transport_upwind (source/ice_transport_driver.F90:634-772) on the resident velocities -------------
// edge velocities and their halo updates (:688-708): E face / N face vectors, in the sig1 / sig2 planes (scratch between calls of
// evpk_principal_stress, which rewrites them whole)
static int edge_velocities(evpk_ctx *c) {
    hipLaunchKernelGGL(k_edge_vel, grid2d(c->s, B2D), B2D, 0, c->stream, c->s, c->cur ? (int)F_STATE1 : (int)F_STATE0, (int)F_SIG1, (int)F_SIG2);
    if (halo(c, F_SIG1, 1, false, true, 0.0, -1, nullptr, false, -1, 0, 2)) return 1;
    return halo(c, F_SIG2, 1, false, true, 0.0, -1, nullptr, false, -1, 0, 3);
}

extern "C" int evpk_transport_upwind(evpk_ctx *c, double dt, int32_t narr, double *works) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !works || narr < 1) return 1;
    if (!c->uploaded) FAIL(c, "evpk_transport_upwind: no velocities on the device (run evp first)");
    if (!c->have_lengths) FAIL(c, "evpk_transport_upwind needs HTN and HTE in evpk_geom");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = mask_elems(s), nblk = (size_t)c->nyb * c->nxb, n = (size_t)c->nblocks * narr * nblk;
    if (!c->tp_a) {
        HIPCHK(c, hipMalloc(&c->tp_a, sizeof(double) * np));
        HIPCHK(c, hipMalloc(&c->tp_b, sizeof(double) * np));
        HIPCHK(c, hipMemsetAsync(c->tp_a, 0, sizeof(double) * np, c->stream));
        HIPCHK(c, hipMemsetAsync(c->tp_b, 0, sizeof(double) * np, c->stream));
    }
    if (edge_velocities(c)) return 1;
    double *dev = nullptr;
    std::vector<HostArr> arr = {{works, n, &dev, true}};
    if (stage_in(c, arr)) return 1;
    const dim3 b(64), g = block_grid(c);
    for (int a = 0; a < narr; a++) {       // upwind_field (:1667-1687), one array at a time through two scratch planes
        LAUNCH_BLOCKS(k_gather_plane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)(dev + (size_t)a * nblk),
                           (size_t)narr * nblk, c->tp_a);
        hipLaunchKernelGGL(k_upwind, dim3((s.nxl + 63) / 64, (s.nyl + 3) / 4), B2D, 0, c->stream, s, dt, (int)F_SIG1, (int)F_SIG2,
                           (const double *)c->tp_a, c->tp_b);
        LAUNCH_BLOCKS(k_scatter_plane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)c->tp_b,
                           dev + (size_t)a * nblk, (size_t)narr * nblk);
    }
    HIPCHK(c, hipGetLastError());
    if (stage_out(c, arr)) return 1;
    return xp_check(c);
}

static int planes_halo(evpk_ctx *c, double **d_list, const signed char *d_sgn, int n, bool vector);

// the per-tracer tables of UpwState from trcr_depend: tracer INDICES (1-based, 0 = none), not the slots of tracer_tables
static int upw_tables(evpk_ctx *c, UpwState &u, int32_t ntrcr, const int32_t *trcr_depend, int32_t nt_Tsfc, int32_t nt_alvl, int32_t nt_apnd,
                      int32_t nt_fbri, int32_t tr_pond_cesm, int32_t tr_pond_lvl, int32_t tr_pond_topo) {
    for (int it = 1; it <= ntrcr; it++) {
        const int dep = trcr_depend[it - 1], k = it - 1;
        // state_to_work (:1435-1497), its branches in the reference's order (the pond branch as written: `a .and. cesm .or. topo`)
        u.base[k] = -1; u.m1[k] = 0; u.m2[k] = 0;
        if (dep == 0) u.base[k] = 0;
        else if (dep == 1) u.base[k] = 1;
        else if (dep == 2) u.base[k] = 2;
        else if (nt_alvl > 0 && dep == 2 + nt_alvl) { u.base[k] = 0; u.m1[k] = (signed char)nt_alvl; }
        else if ((nt_apnd > 0 && dep == 2 + nt_apnd && tr_pond_cesm) || tr_pond_topo) {
            if (nt_apnd < 1) FAIL(c, "evpk_transport_upwind_state: tr_pond_topo without nt_apnd");
            u.base[k] = 0; u.m1[k] = (signed char)nt_apnd;
        }
        else if (nt_apnd > 0 && dep == 2 + nt_apnd && tr_pond_lvl) {
            if (nt_alvl < 1) FAIL(c, "evpk_transport_upwind_state: tr_pond_lvl without nt_alvl");
            u.base[k] = 0; u.m1[k] = (signed char)nt_alvl; u.m2[k] = (signed char)nt_apnd;
        }
        else if (nt_fbri > 0 && dep == 2 + nt_fbri) { u.base[k] = 1; u.m1[k] = (signed char)nt_fbri; }
        // compute_tracers (ice_itd.F90:1411-1497)
        u.rule[k] = -1; u.d1[k] = 0; u.d2[k] = 0;
        if (it == nt_Tsfc) u.rule[k] = 0;
        else if (dep == 0) u.rule[k] = 1;
        else if (dep == 1) u.rule[k] = 2;
        else if (dep == 2) u.rule[k] = 3;
        else if (nt_alvl > 0 && dep == 2 + nt_alvl) { u.rule[k] = 4; u.d1[k] = (signed char)nt_alvl; }
        else if (nt_apnd > 0 && dep == 2 + nt_apnd && (tr_pond_cesm || tr_pond_topo)) { u.rule[k] = 4; u.d1[k] = (signed char)nt_apnd; }
        else if (nt_apnd > 0 && dep == 2 + nt_apnd && tr_pond_lvl) { u.rule[k] = 5; u.d1[k] = (signed char)nt_alvl; u.d2[k] = (signed char)nt_apnd; }
        else if (nt_fbri > 0 && dep == 2 + nt_fbri) { u.rule[k] = 6; u.d1[k] = (signed char)nt_fbri; }
        for (int m : {(int)u.m1[k], (int)u.m2[k], (int)u.d1[k], (int)u.d2[k]})
            if (m > ntrcr) FAIL(c, "evpk_transport_upwind_state: tracer %d hangs on tracer %d, beyond ntrcr", it, m);
    }
    return 0;
}

// ---- transport_upwind with the state transforms (state_to_work, work_to_state + compute_tracers, bound_state) -----------------
extern "C" int evpk_transport_upwind_state(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                                           int32_t nt_Tsfc, int32_t nt_alvl, int32_t nt_apnd, int32_t nt_fbri, int32_t tr_pond_cesm,
                                           int32_t tr_pond_lvl, int32_t tr_pond_topo, double Tocnfrz, double *aice0, double *aicen, double *vicen,
                                           double *vsnon, double *trcrn) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !aice0 || !aicen || !vicen || !vsnon || ncat < 1 || ntrcr < 0 || ntrcr_dim < ntrcr || (ntrcr > 0 && (!trcrn || !trcr_depend))) return 1;
    if (!c->uploaded) FAIL(c, "evpk_transport_upwind_state: no velocities on the device (run evp first)");
    if (!c->have_lengths) FAIL(c, "evpk_transport_upwind_state needs HTN and HTE in evpk_geom");
    if (ntrcr > UW_MAXT) FAIL(c, "evpk_transport_upwind_state: ntrcr = %d exceeds %d", ntrcr, UW_MAXT);
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    UpwState u{};
    u.ncat = ncat; u.ntrcr = ntrcr; u.ntrcr_dim = ntrcr_dim; u.nt_Tsfc = nt_Tsfc; u.nt_fbri = nt_fbri; u.Tocnfrz = Tocnfrz;
    if (upw_tables(c, u, ntrcr, trcr_depend, nt_Tsfc, nt_alvl, nt_apnd, nt_fbri, tr_pond_cesm, tr_pond_lvl, tr_pond_topo)) return 1;
    if (c->check_only) return 0;
    const size_t np = mask_elems(s), nblk = (size_t)c->nyb * c->nxb, N = (size_t)c->nblocks * nblk;
    const int nq = 3 + ntrcr;
    // planes: one input plane, nq output planes of a category
    HIPCHK(c, grow(c, c->uw_pool, c->uw_pool_n, (size_t)(nq + 1) * np, true));
    if (!c->uw_tab) { HIPCHK(c, hipMalloc(&c->uw_tab, sizeof(double *) * (UW_MAXT + 4))); HIPCHK(c, hipMalloc(&c->uw_sgn, UW_MAXT + 4)); }
    std::vector<double *> tab(nq);
    for (int q = 0; q < nq; q++) tab[q] = c->uw_pool + (size_t)(q + 1) * np;
    std::vector<signed char> sg(nq, 1);
    HIPCHK(c, hipMemcpyAsync(c->uw_tab, tab.data(), sizeof(double *) * nq, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->uw_sgn, sg.data(), nq, hipMemcpyHostToDevice, c->stream));
    double *d_aice0 = nullptr;
    std::vector<HostArr> arr = {{aice0, N, &d_aice0, true}, {aicen, N * ncat, &u.aicen, true}, {vicen, N * ncat, &u.vicen, true},
                                {vsnon, N * ncat, &u.vsnon, true}, {trcrn, ntrcr ? N * ncat * ntrcr_dim : 0, &u.trcrn, true}};
    if (stage_in(c, arr)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (tab, sg and staged caller arrays are pageable)
    if (edge_velocities(c)) return 1;
    const dim3 g2 = grid2d(s, B2D), b(64), g = block_grid(c), gu((s.nxl + 63) / 64, (s.nyl + 3) / 4);
    double *pin = c->uw_pool;
    // ghost cells that border an eliminated land block: bound_state's halo update writes its fill (0) into the STATE arrays
    // there (mpi/ice_boundary.F90 srcBlock == 0), not compute_tracers of an empty cell -- the coverage tells k_upw_scatter which they are
    int fcov;
    if (cover_plane(c, F_WORK1, fcov)) return 1;
    // aice0: physical cells only (no halo update in the reference)
    LAUNCH_BLOCKS(k_gather_plane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)d_aice0, nblk, pin);
    hipLaunchKernelGGL(k_upwind, gu, B2D, 0, c->stream, s, dt, (int)F_SIG1, (int)F_SIG2, (const double *)pin, tab[0]);
    LAUNCH_BLOCKS(k_scatter_plane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)tab[0], d_aice0, nblk);
    for (int n = 0; n < ncat; n++) {
        for (int q = 0; q < nq; q++) {
            LAUNCH_BLOCKS(k_upw_gather, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, u, n, q, pin);
            hipLaunchKernelGGL(k_upwind, gu, B2D, 0, c->stream, s, dt, (int)F_SIG1, (int)F_SIG2, (const double *)pin, tab[q]);
        }
        if (planes_halo(c, c->uw_tab, c->uw_sgn, nq, false)) return 1;             // bound_state
        LAUNCH_BLOCKS(k_upw_scatter, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, u, n, (double *const *)c->uw_tab,
                           c->ew == EVPK_BND_CYCLIC ? 1 : 0, c->ns == EVPK_BND_TRIPOLE ? 1 : 0, fcov);
    }
    // F_WORK1 is evp's T-grid wind plane: k_prep1a leaves tiles without input data that were inactive at the previous evp
    // untouched on the understanding that they hold zeros, and k_to_ugrid4 averages them into strairx of U cells on a tile border
    // (round 4's advisor finding: the coverage's 1.0 stayed behind).  EVPK_DEBUG_KEEP_COVER=1 leaves it (the regression test's proof that it bites)
    if (fcov >= 0 && !(getenv("EVPK_DEBUG_KEEP_COVER") && atoi(getenv("EVPK_DEBUG_KEEP_COVER"))))
        hipLaunchKernelGGL(k_fill_plane, g2, B2D, 0, c->stream, s, (int)F_WORK1, 0.0);
    HIPCHK(c, hipGetLastError());
    if (stage_out(c, arr)) return 1;
    return xp_check(c);
}

// the per-tracer tables acc / rule / d1 / d2 / slot of RidgeArgs and ItdArgs from trcr_depend: how aicen * trcrn is built (ice_mechred.F90
// :1456-1513, shift_ice ice_itd.F90:919-975, aggregate :348-433) and compute_tracers (:1407-1499), after the checks of the tracer indices both
// share.  t.nt_Tsfc > 0: compute_tracers asks for nt_Tsfc first (:1408); nt_vlvl: ridge_ice's own index
template <class Args> static int tracer_tables(evpk_ctx *c, const char *who, Args &A, int32_t ntrcr, const int32_t *trcr_depend, const evpk_itd_tracers &t,
                                               int32_t nt_vlvl = 0) {
    const int nts[] = {t.nt_Tsfc, t.nt_qice, t.nt_qsno, t.nt_alvl, nt_vlvl, t.nt_apnd, t.nt_hpnd, t.nt_fbri};
    for (int q : nts) if (q < 0 || q > ntrcr) FAIL(c, "%s: tracer index %d not in 0..ntrcr = %d", who, q, ntrcr);
    if (t.nilyr < 0 || (t.nilyr > 0 && (t.nt_qice < 1 || t.nt_qice + t.nilyr - 1 > ntrcr))) FAIL(c, "%s: nt_qice / nilyr beyond ntrcr", who);
    if (t.nslyr < 0 || (t.nslyr > 0 && (t.nt_qsno < 1 || t.nt_qsno + t.nslyr - 1 > ntrcr))) FAIL(c, "%s: nt_qsno / nslyr beyond ntrcr", who);
    if (t.tr_pond_topo && (t.nt_apnd < 1 || t.nt_hpnd < 1)) FAIL(c, "%s: tr_pond_topo without nt_apnd / nt_hpnd", who);
    if (t.tr_pond_lvl && t.nt_apnd > 0 && t.nt_alvl < 1) FAIL(c, "%s: tr_pond_lvl without nt_alvl", who);
    const bool pond_at = t.tr_pond_cesm || t.tr_pond_topo;
    for (int it = 1; it <= ntrcr; it++) {
        const int dep = trcr_depend[it - 1], k = it - 1;
        A.acc[k] = -1; A.rule[k] = -1; A.d1[k] = 0; A.d2[k] = 0; A.slot[k] = 0;
        if (dep == 0) { A.acc[k] = 0; A.rule[k] = 1; }
        else if (dep == 1) { A.acc[k] = 1; A.rule[k] = 2; }
        else if (dep == 2) { A.acc[k] = 2; A.rule[k] = 3; }
        else if (t.nt_alvl > 0 && dep == 2 + t.nt_alvl) { A.acc[k] = 3; A.rule[k] = 4; A.d1[k] = 1; }
        else if (t.nt_apnd > 0 && dep == 2 + t.nt_apnd && pond_at) { A.acc[k] = 4; A.rule[k] = 4; A.d1[k] = 2; }
        else if (t.nt_apnd > 0 && dep == 2 + t.nt_apnd && t.tr_pond_lvl) { A.acc[k] = 5; A.rule[k] = 5; A.d1[k] = 1; A.d2[k] = 2; }
        else if (t.nt_fbri > 0 && dep == 2 + t.nt_fbri) { A.acc[k] = 6; A.rule[k] = 6; A.d1[k] = 3; }
        if (it == t.nt_Tsfc) A.rule[k] = 0;
        if (it == t.nt_alvl) A.slot[k] = 1;
        else if (it == t.nt_apnd) A.slot[k] = 2;
        else if (it == t.nt_fbri) A.slot[k] = 3;
    }
    return 0;
}

// The first check of the entry points of step_dynamics' second half, which run on x-slab ranks: a context of several ranks on which
// nothing collective has happened yet is refused before any argument is read; a rank without a block column has nothing to do and is in
// no exchange
#define RANKS_ENTRY(c, who)                                                                                                  \
    do {                                                                                                                     \
        if ((c)->nranks > 1 && !(c)->connected) FAIL(c, who ": nranks = %d: the context is not connected yet (evpk_connect)", (c)->nranks); \
        if ((c)->idle) return 0;                                                                                             \
    } while (0)

// ---- ridge_ice (source/ice_mechred.F90:101-746) on the caller's state arrays (kernels in evpk_ridge.hip) ----
extern "C" int evpk_ridge_ice(evpk_ctx *c, double dt, int32_t ndtd, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                              const evpk_ridge_tracers *t, const double *hin_max, const double *rdg_conv, const double *rdg_shear, double *aice0,
                              double *aicen, double *vicen, double *vsnon, double *trcrn, evpk_ridge_diag *diag, int32_t stop[4]) {
    if (!c) return 1;
    if (stop) stop[0] = stop[1] = stop[2] = stop[3] = 0;
    RANKS_ENTRY(c, "evpk_ridge_ice");
    if (!t || !hin_max || !aice0 || !aicen || !vicen || !vsnon || !stop || ntrcr < 0 || ntrcr_dim < ntrcr || (ntrcr > 0 && (!trcrn || !trcr_depend)))
        FAIL(c, "evpk_ridge_ice: a required argument is missing");
    if (!c->connected) FAIL(c, "evpk_ridge_ice: the context is not connected yet (evpk_connect)");
    if (!c->have_params) FAIL(c, "evpk_ridge_ice: evpk_set_params has not been called (krdg_partic, krdg_redist, mu_rdg, rhos)");
    if (!(dt > 0.0) || ndtd < 1) FAIL(c, "evpk_ridge_ice: dt = %g, ndtd = %d", dt, ndtd);
    if (ncat < 1 || ncat > MAXCAT) FAIL(c, "evpk_ridge_ice: ncat = %d not in 1..%d", ncat, MAXCAT);
    if (ntrcr > RG_MAXT) FAIL(c, "evpk_ridge_ice: ntrcr = %d exceeds %d", ntrcr, RG_MAXT);
    if (c->p.krdg_redist == 0)
        FAIL(c, "evpk_ridge_ice: krdg_redist = 0 is not supported: the reference's ridge_shift reads hrmax with the index of its compressed "
                "list of ridging cells (ice_mechred.F90:1724-1725), so its result depends on which other cells of the block ridge");
    if (c->p.krdg_partic != 0 && c->p.krdg_partic != 1) FAIL(c, "evpk_ridge_ice: krdg_partic = %d", c->p.krdg_partic);
    if ((rdg_conv == nullptr) != (rdg_shear == nullptr)) FAIL(c, "evpk_ridge_ice: rdg_conv and rdg_shear must both be given or both be NULL");
    if (!rdg_conv && !(c->prepped && c->ksub >= c->p.ndte))
        FAIL(c, "evpk_ridge_ice: rdg_conv = NULL needs the deformation rates of a finished evp / eap on the device");
    // (ridge_ice's compute_tracers runs without nt_Tsfc: a surface temperature is an ordinary area tracer here)
    evpk_itd_tracers ti{};
    ti.nt_qsno = t->nt_qsno; ti.nslyr = t->nslyr; ti.nt_alvl = t->nt_alvl; ti.nt_apnd = t->nt_apnd; ti.nt_hpnd = t->nt_hpnd; ti.nt_fbri = t->nt_fbri;
    ti.tr_pond_cesm = t->tr_pond_cesm; ti.tr_pond_lvl = t->tr_pond_lvl; ti.tr_pond_topo = t->tr_pond_topo;
    RidgeArgs A{};
    if (tracer_tables(c, "evpk_ridge_ice", A, ntrcr, trcr_depend, ti, t->nt_vlvl)) return 1;
    if (!c->nblocks || c->check_only) return 0;
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    A.ncat = ncat; A.ntrcr = ntrcr; A.ntrcr_dim = ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb;
    A.nt_qsno = t->nt_qsno; A.nslyr = t->nslyr; A.nt_alvl = t->nt_alvl; A.nt_vlvl = t->nt_vlvl; A.nt_apnd = t->nt_apnd; A.nt_hpnd = t->nt_hpnd;
    A.nt_fbri = t->nt_fbri; A.tr_pond_topo = t->tr_pond_topo ? 1 : 0;
    A.dt = dt; A.dti_thermo = 1.0 / (ndtd * dt);
    for (int n = 0; n <= ncat; n++) A.hin_max[n] = hin_max[n];
    A.hin_max[ncat] = 1.0e8;
    const size_t nblk = (size_t)c->nyb * c->nxb, nb = (size_t)c->nblocks, N = nb * nblk;
    // the caller's arrays: in place where the device sees them, else through a staging copy (up, and down again at the end)
    evpk_ridge_diag dg{};
    if (diag) dg = *diag;
    const size_t n2 = N, n3 = N * ncat;
    std::vector<HostArr> arr = {
        {aice0, n2, &A.aice0, true}, {aicen, n3, &A.aicen, true}, {vicen, n3, &A.vicen, true}, {vsnon, n3, &A.vsnon, true},
        {ntrcr ? trcrn : nullptr, n3 * ntrcr_dim, &A.trcrn, true}, {rdg_conv, n2, &A.rdg_conv, false}, {rdg_shear, n2, &A.rdg_shear, false},
        {dg.dardg1dt, n2, &A.dardg1dt, true}, {dg.dardg2dt, n2, &A.dardg2dt, true}, {dg.dvirdgdt, n2, &A.dvirdgdt, true}, {dg.opening, n2, &A.opening, true},
        {dg.fpond, n2, &A.fpond, true}, {dg.fresh, n2, &A.fresh, true}, {dg.fhocn, n2, &A.fhocn, true},
        {dg.dardg1ndt, n3, &A.dardg1ndt, true}, {dg.dardg2ndt, n3, &A.dardg2ndt, true}, {dg.dvirdgndt, n3, &A.dvirdgndt, true},
        {dg.aparticn, n3, &A.aparticn, true}, {dg.krdgn, n3, &A.krdgn, true}, {dg.araftn, n3, &A.araftn, true}, {dg.vraftn, n3, &A.vraftn, true},
        {dg.aredistn, n3, &A.aredistn, true}, {dg.vredistn, n3, &A.vredistn, true}};
    if (stage_in(c, arr)) return 1;
    const size_t nflags = (size_t)(RG_NITER + 1) * nb;
    HIPCHK(c, grow(c, c->rg_pool, c->rg_pool_n, RidgePool::planes(ncat) * N));
    HIPCHK(c, grow(c, c->rg_mask, c->rg_mask_n, N));
    HIPCHK(c, grow(c, c->rg_flags, c->rg_flags_n, nflags));
    if (!c->rg_ctl) HIPCHK(c, hipMalloc(&c->rg_ctl, sizeof(RidgeCtl)));
    RidgeCtl h{};
    h.key = ~0ull;
    HIPCHK(c, hipMemcpyAsync(c->rg_ctl, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rg_flags, 0, sizeof(int) * nflags, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (h and staged caller arrays are pageable)
    RidgePool P{c->rg_pool, c->rg_mask, N, ncat};
    const dim3 b(64), g = block_grid(c);
    int reason = 0, iters = 0;
    for (int iter = 1; iter <= RG_NITER && !reason; iter++) {
        with_ncat(ncat, [&](auto NC) {
            constexpr int nc = decltype(NC)::value;
            hipLaunchKernelGGL(k_ridge_weights<nc>, g, b, 0, c->stream, s, c->p, (const BlockDesc *)c->d_bd, A, P, iter, c->rg_flags, c->nblocks, c->rg_ctl);
            hipLaunchKernelGGL(k_ridge_tracers<nc>, g, b, 0, c->stream, s, (const BlockDesc *)c->d_bd, A, P, iter, (const int *)c->rg_flags, c->nblocks);
        });
        HIPCHK(c, hipGetLastError());
        // what the host learns per iteration: the stop key and whether any block repeats
        HIPCHK(c, hipMemcpyAsync(&h, c->rg_ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        iters = iter;
        if (h.key != ~0ull) reason = ((h.key >> 40) & 0xf) == 0 ? RG_STOP_AICE0 : RG_STOP_ARDG;
        else if (!h.any[iter]) break;
        else if (iter == RG_NITER) reason = RG_STOP_NITER;
    }
    if (!reason) {
        hipLaunchKernelGGL(k_ridge_diag, g, b, 0, c->stream, s, (const BlockDesc *)c->d_bd, A, P, c->rg_ctl);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&h, c->rg_ctl, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (h.key != ~0ull) reason = RG_STOP_ASUM;
    }
    if (reason == RG_STOP_NITER) {          // the first block that still repeats
        std::vector<int> fl(nb);
        HIPCHK(c, hipMemcpy(fl.data(), c->rg_flags + (size_t)RG_NITER * nb, sizeof(int) * nb, hipMemcpyDeviceToHost));
        stop[0] = reason;
        for (size_t q = 0; q < nb; q++) if (fl[q]) { stop[1] = (int32_t)q + 1; break; }
    } else if (reason) {
        const size_t o = (size_t)(h.key & 0xffffffffull);
        stop[0] = reason; stop[1] = (int32_t)(h.key >> 44) + 1; stop[2] = (int32_t)(o % c->nxb) + 1; stop[3] = (int32_t)(o / c->nxb) + 1;
    }
    (void)iters;
    if (stage_out(c, arr)) return 1;
    return reason ? EVPK_RIDGE_STOP : 0;
}

// ---- cleanup_itd and aggregate (source/ice_itd.F90:1514-1769, :246-458) on the caller's state arrays: the rest of step_ridge / step_dynamics
// (kernels in evpk_itd.hip) ----
// the tracer indices and per-tracer tables of ItdArgs
static int itd_tables(evpk_ctx *c, const char *who, ItdArgs &A, int32_t ntrcr, const int32_t *trcr_depend, const evpk_itd_tracers *t) {
    if (tracer_tables(c, who, A, ntrcr, trcr_depend, *t)) return 1;
    A.nt_Tsfc = t->nt_Tsfc; A.nt_qice = t->nt_qice; A.nilyr = t->nilyr; A.nt_qsno = t->nt_qsno; A.nslyr = t->nslyr; A.nt_alvl = t->nt_alvl;
    A.nt_apnd = t->nt_apnd; A.nt_hpnd = t->nt_hpnd; A.nt_fbri = t->nt_fbri; A.tr_pond_topo = t->tr_pond_topo ? 1 : 0; A.tr_brine = t->tr_brine ? 1 : 0;
    return 0;
}

extern "C" int evpk_cleanup_itd(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                                const evpk_itd_tracers *t, const double *hin_max, const evpk_itd_constants *k, int32_t tr_aero, int32_t nbtrcr,
                                int32_t heat_capacity, double *aicen, double *vicen, double *vsnon, double *trcrn, double *aice0, double *aice,
                                double *fpond, double *fresh, double *fsalt, double *fhocn, int32_t *first_ice, int32_t stop[4]) {
    if (!c) return 1;
    if (stop) stop[0] = stop[1] = stop[2] = stop[3] = 0;
    RANKS_ENTRY(c, "evpk_cleanup_itd");
    if (!t || !hin_max || !k || !aice0 || !aice || !aicen || !vicen || !vsnon || !stop || ntrcr < 0 || ntrcr_dim < ntrcr ||
        (ntrcr > 0 && (!trcrn || !trcr_depend)))
        FAIL(c, "evpk_cleanup_itd: a required argument is missing");
    if (!c->connected) FAIL(c, "evpk_cleanup_itd: the context is not connected yet (evpk_connect)");
    if (!c->have_params) FAIL(c, "evpk_cleanup_itd: evpk_set_params has not been called (rhoi, rhos)");
    if (!(dt > 0.0)) FAIL(c, "evpk_cleanup_itd: dt = %g", dt);
    if (ncat < 1 || ncat > MAXCAT) FAIL(c, "evpk_cleanup_itd: ncat = %d not in 1..%d", ncat, MAXCAT);
    if (ntrcr > RG_MAXT) FAIL(c, "evpk_cleanup_itd: ntrcr = %d exceeds %d", ntrcr, RG_MAXT);
    if (tr_aero) FAIL(c, "evpk_cleanup_itd: aerosol tracers (tr_aero) are not supported: faero_ocn cannot be passed");
    if (nbtrcr > 0) FAIL(c, "evpk_cleanup_itd: nbtrcr = %d: bgc tracers are not supported: flux_bio cannot be passed", nbtrcr);
    if (!heat_capacity) FAIL(c, "evpk_cleanup_itd: heat_capacity = .false. (zerolayer_check) is not supported");
    if (k->puny != 1.0e-11) FAIL(c, "evpk_cleanup_itd: puny = %g: compute_tracers on the device is built with 1e-11", k->puny);
    if (c->nblocks >= 65536) FAIL(c, "evpk_cleanup_itd: %d blocks exceed the stop key", c->nblocks);
    ItdArgs A{};
    if (itd_tables(c, "evpk_cleanup_itd", A, ntrcr, trcr_depend, t)) return 1;
    if (ntrcr > 0 && t->nt_Tsfc < 1) FAIL(c, "evpk_cleanup_itd: nt_Tsfc is required (zap_small_areas resets it)");
    if (!c->nblocks || c->check_only) return 0;
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    A.ncat = ncat; A.ntrcr = ntrcr; A.ntrcr_dim = ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb;
    A.dt = dt; A.Tocnfrz = k->Tocnfrz; A.salinity = k->ice_ref_salinity; A.hs_min = k->hs_min; A.cp_ice = k->cp_ice; A.Lfresh = k->Lfresh;
    A.Tmin = k->Tmin; A.puny = k->puny; A.rhoi = c->p.rhoi; A.rhos = c->p.rhos;
    for (int n = 0; n <= ncat; n++) A.hin_max[n] = hin_max[n];
    const size_t nb = (size_t)c->nblocks, N = nb * c->nyb * c->nxb;
    std::vector<HostArr> arr = {
        {aicen, N * ncat, &A.aicen, true}, {vicen, N * ncat, &A.vicen, true}, {vsnon, N * ncat, &A.vsnon, true},
        {ntrcr ? trcrn : nullptr, N * ncat * ntrcr_dim, &A.trcrn, true}, {aice0, N, &A.aice0, true}, {aice, N, &A.aice, true},
        {fpond, N, &A.fpond, true}, {fresh, N, &A.fresh, true}, {fsalt, N, &A.fsalt, true}, {fhocn, N, &A.fhocn, true},
        {first_ice, N * ncat, &A.first_ice, true}};
    if (stage_in(c, arr)) return 1;
    HIPCHK(c, grow(c, c->itd_bmask, c->itd_bmask_n, nb));
    if (!c->itd_key) HIPCHK(c, hipMalloc(&c->itd_key, sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->itd_bmask, 0, sizeof(unsigned) * nb, c->stream));
    HIPCHK(c, hipMemsetAsync(c->itd_key, 0xff, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    const dim3 b(64), g = block_grid(c);
    with_ncat(ncat, [&](auto NC) {
        constexpr int nc = decltype(NC)::value;
        hipLaunchKernelGGL(k_itd_scan<nc>, g, b, 0, c->stream, s, (const BlockDesc *)c->d_bd, A, c->itd_bmask, c->itd_key);
        hipLaunchKernelGGL(k_itd_shift<nc>, g, b, 0, c->stream, s, (const BlockDesc *)c->d_bd, A, (const unsigned *)c->itd_bmask);
        hipLaunchKernelGGL(k_itd_zap<nc>, g, b, 0, c->stream, s, (const BlockDesc *)c->d_bd, A, (const unsigned *)c->itd_bmask, c->itd_key);
    });
    HIPCHK(c, hipGetLastError());
    unsigned long long key = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&key, c->itd_key, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    if (stage_out(c, arr)) return 1;
    if (key == ~0ull) return 0;
    const int stage = (int)((key >> 40) & 0xff), sub = (int)((key >> 32) & 0xff);
    const unsigned code = (unsigned)(key & 0xffffffffull);
    const bool rebin = stage >= 1 && stage < 2 * ncat;
    const size_t o = (stage == 0 || rebin) ? (size_t)(0xffffffffu - code) : (size_t)code;
    stop[0] = stage == 0 ? ITD_STOP_BOUNDS : rebin ? ITD_STOP_NEG_DAICE + sub : stage == 2 * ncat ? ITD_STOP_NEG_AICEN : ITD_STOP_EXCESS;
    stop[1] = (int32_t)(key >> 48) + 1; stop[2] = (int32_t)(o % c->nxb) + 1; stop[3] = (int32_t)(o / c->nxb) + 1;
    return EVPK_ITD_STOP;
}

// ---- linear_itd as step_therm2 calls it (ice_step_mod.F90:821-871, ice_therm_itd.F90:69-859) on the caller's state arrays ----
extern "C" int evpk_linear_itd(evpk_ctx *c, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend, const evpk_itd_tracers *t,
                               const double *hin_max, double hi_min, const evpk_itd_constants *k, const double *aicen_init,
                               const double *vicen_init, double *aicen, double *vicen, double *vsnon, double *trcrn, double *aice, double *aice0,
                               double *fpond, int32_t stop[4]) {
    if (!c) return 1;
    if (stop) stop[0] = stop[1] = stop[2] = stop[3] = 0;
    RANKS_ENTRY(c, "evpk_linear_itd");
    if (!t || !hin_max || !k || !aicen_init || !vicen_init || !aice0 || !aice || !aicen || !vicen || !vsnon || !stop || ntrcr < 0 ||
        ntrcr_dim < ntrcr || (ntrcr > 0 && (!trcrn || !trcr_depend)))
        FAIL(c, "evpk_linear_itd: a required argument is missing");
    if (!c->connected) FAIL(c, "evpk_linear_itd: the context is not connected yet (evpk_connect)");
    if (!c->have_params) FAIL(c, "evpk_linear_itd: evpk_set_params has not been called (rhos)");
    if (ncat < 1 || ncat > MAXCAT) FAIL(c, "evpk_linear_itd: ncat = %d not in 1..%d", ncat, MAXCAT);
    if (ntrcr > RG_MAXT) FAIL(c, "evpk_linear_itd: ntrcr = %d exceeds %d", ntrcr, RG_MAXT);
    if (k->puny != 1.0e-11) FAIL(c, "evpk_linear_itd: puny = %g: compute_tracers on the device is built with 1e-11", k->puny);
    if (c->nblocks >= 65536) FAIL(c, "evpk_linear_itd: %d blocks exceed the stop key", c->nblocks);
    ItdArgs A{};
    if (itd_tables(c, "evpk_linear_itd", A, ntrcr, trcr_depend, t)) return 1;
    if (ntrcr > 0 && t->nt_Tsfc < 1) FAIL(c, "evpk_linear_itd: nt_Tsfc is required (compute_tracers resets it to Tocnfrz)");
    if (t->tr_pond_topo && !fpond) FAIL(c, "evpk_linear_itd: tr_pond_topo needs fpond");
    if (!c->nblocks || c->check_only) return 0;
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    A.ncat = ncat; A.ntrcr = ntrcr; A.ntrcr_dim = ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb;
    A.Tocnfrz = k->Tocnfrz; A.Lfresh = k->Lfresh; A.puny = k->puny; A.rhos = c->p.rhos;
    for (int n = 0; n < ncat; n++) A.hin_max[n] = hin_max[n];
    A.hin_max[ncat] = 999.9;                              // ice_therm_itd.F90:208 (the caller's array is not written)
    LitdArgs L{};
    L.hi_min = hi_min;
    const size_t nb = (size_t)c->nblocks, N = nb * c->nyb * c->nxb;
    std::vector<HostArr> arr = {
        {aicen_init, N * ncat, &L.aicen_init, false}, {vicen_init, N * ncat, &L.vicen_init, false},
        {aicen, N * ncat, &A.aicen, true}, {vicen, N * ncat, &A.vicen, true}, {vsnon, N * ncat, &A.vsnon, true},
        {ntrcr ? trcrn : nullptr, N * ncat * ntrcr_dim, &A.trcrn, true}, {aice, N, &A.aice, true}, {aice0, N, &A.aice0, true},
        {t->tr_pond_topo ? fpond : nullptr, N, &A.fpond, true}};
    if (stage_in(c, arr)) return 1;
    HIPCHK(c, grow(c, c->itd_bmask, c->itd_bmask_n, nb));
    if (!c->itd_key) HIPCHK(c, hipMalloc(&c->itd_key, sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->itd_bmask, 0, sizeof(unsigned) * nb, c->stream));
    HIPCHK(c, hipMemsetAsync(c->itd_key, 0xff, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    const dim3 b(64), g = block_grid(c);
    with_ncat(ncat, [&](auto NC) {
        constexpr int nc = decltype(NC)::value;
        hipLaunchKernelGGL(k_litd_scan<nc>, g, b, 0, c->stream, s, (const BlockDesc *)c->d_bd, A, c->itd_bmask);
        hipLaunchKernelGGL(k_litd_remap<nc>, g, b, 0, c->stream, s, (const BlockDesc *)c->d_bd, A, L, (const unsigned *)c->itd_bmask, c->itd_key);
    });
    HIPCHK(c, hipGetLastError());
    unsigned long long key = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&key, c->itd_key, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    if (stage_out(c, arr)) return 1;
    if (key == ~0ull) return 0;
    const size_t o = (size_t)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    stop[0] = ITD_STOP_NEG_DAICE + (int)((key >> 32) & 0xff);
    stop[1] = (int32_t)(key >> 48) + 1; stop[2] = (int32_t)(o % c->nxb) + 1; stop[3] = (int32_t)(o / c->nxb) + 1;
    return EVPK_LITD_STOP;
}

// bound_state (ice_state.F90:173-238): ice_HaloUpdate, centre scalar, of aicen, trcrn(1:ntrcr), vicen, vsnon on the device -- the planes go
// through the scratch state planes and the general update, as evpk_halo_update's do (fill 0 next to an eliminated land block)
static int itd_bound_state(evpk_ctx *c, const ItdArgs &A) {
    const size_t nn = (size_t)c->nyb * c->nxb;
    std::vector<BlockPlane> pl;
    for (int n = 0; n < A.ncat; n++) pl.push_back({A.aicen + (size_t)n * nn, (size_t)A.ncat * nn});
    for (int n = 0; n < A.ncat; n++)
        for (int it = 0; it < A.ntrcr; it++) pl.push_back({A.trcrn + ((size_t)n * A.ntrcr_dim + it) * nn, (size_t)A.ncat * A.ntrcr_dim * nn});
    for (int n = 0; n < A.ncat; n++) pl.push_back({A.vicen + (size_t)n * nn, (size_t)A.ncat * nn});
    for (int n = 0; n < A.ncat; n++) pl.push_back({A.vsnon + (size_t)n * nn, (size_t)A.ncat * nn});
    c->bs_planes = (int)pl.size();
    const int chunk = std::min(c->max_nf, (int)NSTATE);             // (block_planes_halo's: one fold + one ring exchange per chunk)
    c->bs_rounds = c->nranks > 1 ? ((int)pl.size() + chunk - 1) / chunk : 0;
    return block_planes_halo(c, pl, 1, 1, 0.0);          // centre scalars
}

// k_bound_state finds the block of a global cell as (column, row) of a uniform tiling: true of what create_blocks makes -- every block
// starts at a multiple of the block size and is full except in the last column / row
static int remap_block_map(evpk_ctx *c);
static bool bound_direct_ok(evpk_ctx *c) {
    if (!c->bs_uniform) {
        const int bsx = c->nxb - 2, bsy = c->nyb - 2;
        // (x-slab ranks: the same tiling of the global grid on the rank's own block columns, which start the slab)
        bool ok = c->s.j0 == 1 && c->s.nyl == c->s.nyg && (c->nranks > 1 ? (c->s.i0 - 1) % bsx == 0 : (c->s.i0 == 1 && c->s.nxl == c->s.nxg));
        for (int b = 0; ok && b < c->nblocks; b++) {
            const BlockDesc &d = c->bd[b];
            const int ci = (d.iglob_lo - 1) / bsx, cj = (d.jglob_lo - 1) / bsy;
            ok = d.iglob_lo == ci * bsx + 1 && d.jglob_lo == cj * bsy + 1 && d.ihi - d.ilo + 1 == std::min(bsx, c->s.nxg - ci * bsx) &&
                 d.jhi - d.jlo + 1 == std::min(bsy, c->s.nyg - cj * bsy) && d.iglob_lo >= c->s.i0 && d.iglob_lo + (d.ihi - d.ilo) < c->s.i0 + c->s.nxl;
        }
        c->bs_uniform = ok ? 1 : -1;
    }
    return c->bs_uniform > 0;
}

// bound_state in one launch, block array to block array (k_bound_state, evpk_itd.hip): the same cells get the same values as above
static int itd_bound_direct(evpk_ctx *c, const ItdArgs &A) {
    if (remap_block_map(c)) return 1;            // (uploaded once per context: it depends on the decomposition only)
    const size_t nn = (size_t)c->nyb * c->nxb;
    BsArgs B{};
    B.aicen = {A.aicen, (size_t)A.ncat * nn}; B.trcrn = {A.trcrn, (size_t)A.ncat * A.ntrcr_dim * nn};
    B.vicen = {A.vicen, (size_t)A.ncat * nn}; B.vsnon = {A.vsnon, (size_t)A.ncat * nn};
    B.ncat = A.ncat; B.ntrcr = A.ntrcr; B.ntrcr_dim = A.ntrcr_dim; B.nxb = c->nxb; B.nyb = c->nyb; B.nplanes = A.ncat * (3 + A.ntrcr);
    B.nxg = c->s.nxg; B.nyg = c->s.nyg; B.bsx = c->nxb - 2; B.bsy = c->nyb - 2; B.nbx = c->bmap_nbx;
    B.cyclic = c->ew == EVPK_BND_CYCLIC ? 1 : 0; B.tripole = c->ns == EVPK_BND_TRIPOLE ? 1 : 0;
    if (c->nblocks > 65535) FAIL(c, "evpk_bound_state: %d blocks exceed one launch", c->nblocks);
    const dim3 g((4 * (c->nxb + c->nyb) + BS_TX - 1) / BS_TX, c->nblocks, (B.nplanes + BS_PG - 1) / BS_PG);
    LAUNCH_BLOCKS(k_bound_state, g, dim3(BS_TX), 0, c->stream, (const BlockDesc *)c->d_bd, (const int *)c->d_bmap, B);
    HIPCHK(c, hipGetLastError());
    c->bs_rounds = 0; c->bs_planes = B.nplanes;
    return 0;
}

// bound_state across x-slab ranks (k_bound_pack -> one exchange -> k_bound_fill, evpk_itd.hip): every rank packs physical cells only --
// its edge columns for the ring neighbours, its top row for its tripole fold partners -- into ONE message per partner, the ring and the
// fold messages are posted together, and every ghost cell is then filled in one launch.  A message holds up to `ppr` planes; more planes
// take more rounds.  ppr follows from quantities every rank shares (the slot size, wmax, ny_global, the plane count), never from the
// rank's own slab width, so that all ranks post the same exchanges.  A rank whose blocks are all eliminated packs zeros and fills nothing.
static int itd_bound_ranks(evpk_ctx *c, const ItdArgs &A) {
    if (remap_block_map(c)) return 1;
    Slab &s = c->s;
    hipStream_t st = c->stream;
    const int ch = xp_channel(c, st);
    const size_t nn = (size_t)c->nyb * c->nxb;
    BsArgs B{};
    B.aicen = {A.aicen, (size_t)A.ncat * nn}; B.trcrn = {A.trcrn, (size_t)A.ncat * A.ntrcr_dim * nn};
    B.vicen = {A.vicen, (size_t)A.ncat * nn}; B.vsnon = {A.vsnon, (size_t)A.ncat * nn};
    B.ncat = A.ncat; B.ntrcr = A.ntrcr; B.ntrcr_dim = A.ntrcr_dim; B.nxb = c->nxb; B.nyb = c->nyb; B.nplanes = A.ncat * (3 + A.ntrcr);
    B.nxg = s.nxg; B.nyg = s.nyg; B.bsx = c->nxb - 2; B.bsy = c->nyb - 2; B.nbx = c->bmap_nbx;
    B.cyclic = c->ew == EVPK_BND_CYCLIC ? 1 : 0; B.tripole = c->ns == EVPK_BND_TRIPOLE ? 1 : 0;
    if (c->nblocks > 65535) FAIL(c, "evpk_bound_state: %d blocks exceed one launch", c->nblocks);
    // partners: the ring neighbours, then the fold partners that are not among them; what each message holds
    struct Partner { int q; bool w, e, t; };
    std::vector<Partner> P;
    if (c->west >= 0) P.push_back({c->west, true, c->east == c->west, false});
    if (c->east >= 0 && c->east != c->west) P.push_back({c->east, false, true, false});
    if (B.tripole)
        for (int q : c->fold_dst) {
            bool found = false;
            for (Partner &p : P) if (p.q == q) { p.t = true; found = true; }
            if (!found) P.push_back({q, false, false, true});
        }
    if ((int)c->fold_dst.size() > BR_MAXT) FAIL(c, "evpk_bound_state: %d fold partners", (int)c->fold_dst.size());
    // planes per round, the same on every rank
    const size_t unit = (size_t)2 * s.nyg + c->wmax;
    const size_t cap = c->ipc ? c->ipc->slot[ch] / sizeof(double) : c->relay ? c->relay->slot / sizeof(double) : unit * B.nplanes;
    const int ppr = (int)std::min<size_t>((size_t)B.nplanes, cap / unit);
    if (ppr < 1) FAIL(c, "evpk_bound_state: one plane's messages (%zu doubles) do not fit the transport's slot", unit);
    const int rounds = (B.nplanes + ppr - 1) / ppr;
    const size_t msgcap = (size_t)ppr * unit;             // doubles per message buffer
    if (!c->ipc) HIPCHK(c, grow(c, c->br_buf, c->br_buf_n, 2 * P.size() * msgcap));
    auto lsend = [&](size_t k) { return c->br_buf + k * msgcap; };
    auto lrecv = [&](size_t k) { return c->br_buf + (P.size() + k) * msgcap; };
    for (int r = 0; r < rounds; r++) {
        BrArgs R{};
        R.i0 = s.i0; R.i1 = s.i0 + s.nxl - 1; R.p0 = r * ppr; R.np = std::min(ppr, B.nplanes - R.p0);
        const size_t col = (size_t)R.np * s.nyg;
        std::vector<size_t> nsend(P.size()), nrecv(P.size());
        for (size_t k = 0; k < P.size(); k++) {
            const Partner &p = P[k];
            // (peer-mapped: the page of the NEXT message, before the signal / wait turn it)
            double *snd = c->ipc ? ipc_send_ptr(c, ch, p.q, 0) : lsend(k);
            const double *rcv = c->ipc ? ipc_recv_ptr(c, ch, p.q, 0) : lrecv(k);
            const int wq = c->slab_i0[p.q + 1] - c->slab_i0[p.q];
            size_t o = 0;
            if (p.w) { R.toW = snd + o; o += col; }
            if (p.e) { R.toE = snd + o; o += col; }
            if (p.t) { R.toT[R.nT++] = snd + o; o += (size_t)R.np * s.nxl; }
            nsend[k] = o;
            // the partner's message: its W section if this rank is its west neighbour (it is this rank's east one), and so on
            o = 0;
            if (p.e) { R.fromE = rcv + o; o += col; }
            if (p.w) { R.fromW = rcv + o; o += col; }
            if (p.t) { R.fromT[R.nS] = rcv + o; R.t_i0[R.nS] = c->slab_i0[p.q]; R.t_w[R.nS++] = wq; o += (size_t)R.np * wq; }
            nrecv[k] = o;
            if (nsend[k] > msgcap || nrecv[k] > msgcap) FAIL(c, "evpk_bound_state: message larger than its buffer");
        }
        const int ng = (R.np + BS_PG - 1) / BS_PG;
        hipLaunchKernelGGL(k_bound_pack, dim3((std::max(s.nyg, s.nxl) + BS_TX - 1) / BS_TX, 3, ng), dim3(BS_TX), 0, st, (const BlockDesc *)c->d_bd,
                           (const int *)c->d_bmap, B, R);
        HIPCHK(c, hipGetLastError());
        if (c->ipc) {
            for (const Partner &p : P) if (ipc_signal(c, ch, p.q, st)) return 1;
            for (const Partner &p : P) if (ipc_wait(c, ch, p.q, st)) return 1;
        } else if (c->relay) {
            int rc = 0;
            for (size_t k = 0; k < P.size(); k++) rc |= c->relay->send(P[k].q, lsend(k), nsend[k] * 8, st);
            for (size_t k = 0; k < P.size(); k++) rc |= c->relay->recv(P[k].q, lrecv(k), nrecv[k] * 8, st);
            if (rc) FAIL(c, "shared-memory relay: bound_state exchange failed (%s)", rc & 2 ? "timeout" : "copy / size");
        } else {
            NCCLCHK(c, ncclGroupStart());
            ncclResult_t rc = ncclSuccess;
            auto keep = [&](ncclResult_t e) { if (rc == ncclSuccess) rc = e; };
            for (size_t k = 0; k < P.size(); k++) if (nsend[k]) keep(ncclSend(lsend(k), nsend[k], ncclDouble, P[k].q, c->comm, st));
            for (size_t k = 0; k < P.size(); k++) if (nrecv[k]) keep(ncclRecv(lrecv(k), nrecv[k], ncclDouble, P[k].q, c->comm, st));
            const ncclResult_t rce = ncclGroupEnd();
            if (rc != ncclSuccess) FAIL(c, "bound_state exchange: ncclSend/ncclRecv failed: %s", ncclGetErrorString(rc));
            if (rce != ncclSuccess) FAIL(c, "bound_state exchange: ncclGroupEnd failed: %s", ncclGetErrorString(rce));
        }
        const dim3 g((4 * (c->nxb + c->nyb) + BS_TX - 1) / BS_TX, c->nblocks, ng);
        if (g.y) hipLaunchKernelGGL(k_bound_fill, g, dim3(BS_TX), 0, st, (const BlockDesc *)c->d_bd, (const int *)c->d_bmap, B, R);
        HIPCHK(c, hipGetLastError());
    }
    c->bs_rounds = rounds; c->bs_planes = B.nplanes;
    return 0;
}

// EVPK_BOUND_DIRECT=0 (read per call): the plane-by-plane path, the A/B partner and the pinned definition
static bool bound_direct_env() { return env_on("EVPK_BOUND_DIRECT"); }

// bound_state of the device arrays of A by the path the knob and the decomposition select (collective on x-slab ranks).  On one rank a
// decomposition that is not the uniform tiling takes the plane-by-plane path; on several every rank must take the same path, so there
// it is an error
static int itd_bound(evpk_ctx *c, const ItdArgs &A, const char *who) {
    if (!bound_direct_env()) return itd_bound_state(c, A);
    if (!bound_direct_ok(c)) {
        if (c->nranks > 1) FAIL(c, "%s: the blocks are not the uniform tiling of create_blocks (EVPK_BOUND_DIRECT=0 on every rank takes the plane-by-plane path)", who);
        return itd_bound_state(c, A);
    }
    return c->nranks > 1 ? itd_bound_ranks(c, A) : itd_bound_direct(c, A);
}

extern "C" int evpk_bound_state(evpk_ctx *c, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, double *aicen, double *vicen, double *vsnon,
                                double *trcrn) {
    if (!c) return 1;
    RANKS_ENTRY(c, "evpk_bound_state");
    if (!aicen || !vicen || !vsnon || ntrcr < 0 || ntrcr_dim < ntrcr || (ntrcr > 0 && !trcrn)) FAIL(c, "evpk_bound_state: a required argument is missing");
    if (!c->connected) FAIL(c, "evpk_bound_state: the context is not connected yet (evpk_connect)");
    if (ncat < 1 || ncat > MAXCAT) FAIL(c, "evpk_bound_state: ncat = %d not in 1..%d", ncat, MAXCAT);
    if (ntrcr > RG_MAXT) FAIL(c, "evpk_bound_state: ntrcr = %d exceeds %d", ntrcr, RG_MAXT);
    if (!c->nblocks && c->nranks == 1) return 0;          // (a slab rank whose blocks are all eliminated still posts its messages)
    HIPCHK(c, hipSetDevice(c->device));
    const bool direct = bound_direct_env();
    if (direct && !bound_direct_ok(c)) FAIL(c, "evpk_bound_state: the blocks are not the uniform tiling of create_blocks (EVPK_BOUND_DIRECT=0 takes the plane-by-plane path)");
    ItdArgs A{};
    A.ncat = ncat; A.ntrcr = ntrcr; A.ntrcr_dim = ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb;
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb;
    std::vector<HostArr> arr = {{aicen, N * ncat, &A.aicen, true}, {vicen, N * ncat, &A.vicen, true}, {vsnon, N * ncat, &A.vsnon, true},
                                {ntrcr ? trcrn : nullptr, N * ncat * ntrcr_dim, &A.trcrn, true}};
    if (stage_in(c, arr)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    if (itd_bound(c, A, "evpk_bound_state")) return 1;
    if (stage_out(c, arr)) return 1;
    return xp_check(c);
}

extern "C" int evpk_aggregate(evpk_ctx *c, double dt, int32_t bound, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                              const evpk_itd_tracers *t, int32_t nt_iage, double Tocnfrz, double *aicen, double *vicen, double *vsnon, double *trcrn,
                              double *aice, double *vice, double *vsno, double *aice0, double *trcr, double *daidtd, double *dvidtd,
                              double *dagedtd) {
    if (!c) return 1;
    RANKS_ENTRY(c, "evpk_aggregate");
    if (!t || !aice0 || !aice || !vice || !vsno || !aicen || !vicen || !vsnon || ntrcr < 0 || ntrcr_dim < ntrcr ||
        (ntrcr > 0 && (!trcrn || !trcr_depend || !trcr)))
        FAIL(c, "evpk_aggregate: a required argument is missing");
    if (!c->connected) FAIL(c, "evpk_aggregate: the context is not connected yet (evpk_connect)");
    if (!(dt > 0.0)) FAIL(c, "evpk_aggregate: dt = %g", dt);
    if (bound != 0 && bound != 1) FAIL(c, "evpk_aggregate: bound = %d", bound);
    if (ncat < 1 || ncat > MAXCAT) FAIL(c, "evpk_aggregate: ncat = %d not in 1..%d", ncat, MAXCAT);
    if (ntrcr > RG_MAXT) FAIL(c, "evpk_aggregate: ntrcr = %d exceeds %d", ntrcr, RG_MAXT);
    if (nt_iage < 0 || nt_iage > ntrcr) FAIL(c, "evpk_aggregate: nt_iage = %d not in 0..ntrcr = %d", nt_iage, ntrcr);
    ItdArgs A{};
    if (itd_tables(c, "evpk_aggregate", A, ntrcr, trcr_depend, t)) return 1;
    if (c->check_only || (!c->nblocks && !(bound && c->nranks > 1))) return 0;     // (bound_state is collective: a slab rank whose blocks
    Slab &s = c->s;                                                                   // are all eliminated still posts its messages)
    HIPCHK(c, hipSetDevice(c->device));
    A.ncat = ncat; A.ntrcr = ntrcr; A.ntrcr_dim = ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb; A.nt_iage = nt_iage;
    A.dt = dt; A.Tocnfrz = Tocnfrz; A.puny = 1.0e-11;
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb;
    const bool bnd = bound != 0;          // (without bound_state the category arrays are inputs)
    std::vector<HostArr> arr = {
        {aicen, N * ncat, &A.aicen, bnd}, {vicen, N * ncat, &A.vicen, bnd}, {vsnon, N * ncat, &A.vsnon, bnd},
        {ntrcr ? trcrn : nullptr, N * ncat * ntrcr_dim, &A.trcrn, bnd}, {aice0, N, &A.aice0, true}, {aice, N, &A.aice, true},
        {vice, N, &A.vice, true}, {vsno, N, &A.vsno, true}, {ntrcr ? trcr : nullptr, N * ntrcr_dim, &A.trcr, true},
        {daidtd, N, &A.daidtd, true}, {dvidtd, N, &A.dvidtd, true}, {dagedtd, N, &A.dagedtd, true}};
    if (stage_in(c, arr)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    if (bnd && itd_bound(c, A, "evpk_aggregate")) return 1;
    if (c->nblocks)
        with_ncat(ncat, [&](auto NC) {
            hipLaunchKernelGGL(k_itd_aggregate<decltype(NC)::value>, block_grid(c), dim3(64), 0, c->stream, s, (const BlockDesc *)c->d_bd, A);
        });
    HIPCHK(c, hipGetLastError());
    if (stage_out(c, arr)) return 1;
    return xp_check(c);
}

// ---- transport_remap's horizontal_remap (source/ice_transport_remap.F90:309-850) on the resident velocities ----
// grid arrays the EVP path does not hold: dxu, dyu (ice_grid) and hm (the land mask as a real); block arrays, ghost cells current
extern "C" int evpk_remap_init(evpk_ctx *c, const double *dxu, const double *dyu, const double *hm) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !dxu || !dyu || !hm) return 1;
    if (!c->connected) FAIL(c, "evpk_remap_init: the context is not connected yet (evpk_connect)");
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = mask_elems(s), nblk = (size_t)c->nyb * c->nxb, n = (size_t)c->nblocks * nblk;
    if (!c->rm_grid) HIPCHK(c, hipMalloc(&c->rm_grid, sizeof(double) * 3 * np));
    if (!c->rm_bad) HIPCHK(c, hipMalloc(&c->rm_bad, sizeof(unsigned)));
    HIPCHK(c, hipMemsetAsync(c->rm_grid, 0, sizeof(double) * 3 * np, c->stream));
    if (c->stage_n < n) FAIL(c, "evpk_remap_init: staging buffer too small");
    const double *src[3] = {dxu, dyu, hm};
    const dim3 b(64), g((c->nxb + 63) / 64, c->nyb, c->nblocks);
    for (int q = 0; q < 3; q++) {
        const double *dev = (const double *)mapped_alias(src[q], sizeof(double) * n);
        if (!dev) {
            HIPCHK(c, hipMemcpyAsync(c->stage, src[q], sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
            dev = c->stage;
        }
        LAUNCH_BLOCKS(k_gather_plane, g, b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, dev, nblk, c->rm_grid + (size_t)q * np);
        HIPCHK(c, hipStreamSynchronize(c->stream));      // (the staging buffer is reused by the next array)
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// ghost ring of a list of plain planes (centre location; scalars or vectors): one launch on one rank, else through the
// scratch state planes and the general update, max_nf planes at a time
static int planes_halo(evpk_ctx *c, double **d_list, const signed char *d_sgn, int n, bool vector) {
    Slab &s = c->s;
    if (n <= 0) return 0;
    if (c->ns == EVPK_BND_CYCLIC) FAIL(c, "ns_boundary_type cyclic is not supported");
    const int tx = 128;
    if (c->nranks == 1 && !c->force_exchange) {
        hipLaunchKernelGGL(k_planes_halo, dim3((s.nxl + s.nyl + 2 + tx - 1) / tx, n), dim3(tx), 0, c->stream, s, (double *const *)d_list, d_sgn,
                           c->ew == EVPK_BND_CYCLIC ? 1 : 0, c->ns == EVPK_BND_TRIPOLE ? 1 : 0);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    const int nt = 4 * (s.nxl + 2) + 4 * (s.nyl + 2);
    for (int q = 0; q < n; q += c->max_nf) {
        const int nf = std::min(c->max_nf, n - q);
        hipLaunchKernelGGL(k_planes_frame, dim3((nt + tx - 1) / tx), dim3(tx), 0, c->stream, s, (double *const *)(d_list + q), (int)F_STATE2, nf, 0);
        if (halo(c, F_STATE2, nf, false, vector, 0.0)) return 1;
        hipLaunchKernelGGL(k_planes_frame, dim3((nt + tx - 1) / tx), dim3(tx), 0, c->stream, s, (double *const *)(d_list + q), (int)F_STATE2, nf, 1);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// st == nullptr: mm / tm are the caller's aim / trm; else the caller's state arrays (host pointers in *st) through the fused transforms
// block column / row of the global grid -> local block index (-1: not here), for kernels that write a slab cell into the
// caller's block arrays themselves
static int remap_block_map(evpk_ctx *c) {
    if (c->d_bmap) return 0;
    const int bsx = c->nxb - 2, bsy = c->nyb - 2;
    const int nbx = (c->s.nxg - 1) / bsx + 1, nby = (c->s.nyg - 1) / bsy + 1;
    std::vector<int> m((size_t)nbx * nby, -1);
    for (int b = 0; b < c->nblocks; b++)
        m[(size_t)((c->bd[b].jglob_lo - 1) / bsy) * nbx + (c->bd[b].iglob_lo - 1) / bsx] = b;
    HIPCHK(c, hipMalloc(&c->d_bmap, sizeof(int) * m.size()));
    HIPCHK(c, hipMemcpy(c->d_bmap, m.data(), sizeof(int) * m.size(), hipMemcpyHostToDevice));
    c->bmap_nbx = nbx;
    return 0;
}

static int remap_impl(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrace, double *mm, double *tm, const int32_t *tracer_type,
                      const int32_t *depend, const int32_t *has_dependents, int32_t integral_order, int32_t l_dp_midpt,
                      int32_t l_fixed_area, const RemapState *st) {
    if (!c || (!st && !mm) || ncat < 1 || ntrace < 0 || (ntrace > 0 && ((!st && !tm) || !tracer_type || !depend || !has_dependents))) return 1;
    if (!c->uploaded) FAIL(c, "evpk_transport_remap: no velocities on the device (run evp first)");
    if (!c->have_lengths) FAIL(c, "evpk_transport_remap needs HTN and HTE in evpk_geom");
    if (!c->rm_grid) FAIL(c, "evpk_transport_remap: evpk_remap_init has not been called");
    if (l_fixed_area) FAIL(c, "evpk_transport_remap: l_fixed_area = .true. is not supported");
    if (ntrace > RM_MAXT) FAIL(c, "evpk_transport_remap: ntrace = %d exceeds %d", ntrace, RM_MAXT);
    if (mask_elems(c->s) > 0xFFFFFFFFull) FAIL(c, "evpk_transport_remap: a plane of this slab has more than 2^32 cells");   // (k_remap_flux keeps 32-bit cell offsets)
    if (integral_order < 1 || integral_order > 3) FAIL(c, "evpk_transport_remap: integral_order = %d", integral_order);
    RemapTab tb{};
    tb.ncat = ncat; tb.ntrace = ntrace; tb.order = integral_order; tb.midpt = l_dp_midpt ? 1 : 0;
    for (int nt = 0; nt < ntrace; nt++) {
        if (tracer_type[nt] < 1 || tracer_type[nt] > 3) FAIL(c, "evpk_transport_remap: tracer_type(%d) = %d", nt + 1, tracer_type[nt]);
        // a dependent tracer follows the one it depends on (init_transport orders them so, ice_transport_driver.F90:88-125); type 2
        // hangs on a type 1 (hice, hsno or an area tracer), type 3 on a type 2
        if (tracer_type[nt] > 1) {
            if (depend[nt] < 1 || depend[nt] > nt) FAIL(c, "evpk_transport_remap: depend(%d) = %d", nt + 1, depend[nt]);
            const int par = depend[nt] - 1;
            if (tracer_type[par] != tracer_type[nt] - 1)
                FAIL(c, "evpk_transport_remap: tracer %d (type %d) must depend on a type %d tracer", nt + 1, tracer_type[nt], tracer_type[nt] - 1);
            if (tracer_type[nt] == 2 && !has_dependents[par]) FAIL(c, "evpk_transport_remap: has_dependents(%d) is false but tracer %d depends on it", par + 1, nt + 1);
        }
        tb.type[nt] = (signed char)tracer_type[nt]; tb.dep[nt] = (signed char)depend[nt]; tb.has[nt] = has_dependents[nt] ? 1 : 0;
    }
    {   // depth-first order of the dependency forest (RemapTab::ord)
        int m = 0;
        for (int a = 0; a < ntrace; a++) {
            if (tracer_type[a] != 1) continue;
            tb.ord[m++] = (signed char)a;
            for (int b2 = a + 1; b2 < ntrace; b2++) {
                if (tracer_type[b2] != 2 || depend[b2] - 1 != a) continue;
                tb.ord[m++] = (signed char)b2;
                for (int b3 = b2 + 1; b3 < ntrace; b3++)
                    if (tracer_type[b3] == 3 && depend[b3] - 1 == b2) tb.ord[m++] = (signed char)b3;
            }
        }
        if (m != ntrace) FAIL(c, "evpk_transport_remap: the tracer dependencies do not form a forest (%d of %d reached)", m, ntrace);
    }
    if (c->check_only) return 0;
    Slab &s = c->s;
    HIPCHK(c, hipSetDevice(c->device));
    const int ncp = ncat + 1, ntp = ncat * ntrace;
    const size_t np = mask_elems(s), nblk = (size_t)c->nyb * c->nxb;
    const size_t nplanes = (size_t)5 * ncp + (size_t)6 * ntp;
    if (grow(c, c->rm_pool, c->rm_pool_n, nplanes * np, true) != hipSuccess)
        FAIL(c, "evpk_transport_remap: %zu planes of %zu cells do not fit on the device", nplanes, np);
    // pointer tables: [0, nplanes) the planes in RemapPlanes order; then the two halo lists
    //   A (before construct_fields): mm, tm -- scalars;   B: tc -- scalars, then mx, my, tx, ty -- vectors
    std::vector<double *> tab(nplanes);
    for (size_t q = 0; q < nplanes; q++) tab[q] = c->rm_pool + q * np;
    const size_t o_tm = 5 * ncp, o_tc = o_tm + ntp, o_tx = o_tc + ntp, o_ty = o_tx + ntp;
    std::vector<double *> lst;
    std::vector<signed char> sg;
    for (int q = 0; q < ncp; q++) { lst.push_back(tab[q]); sg.push_back(1); }
    for (int q = 0; q < ntp; q++) { lst.push_back(tab[o_tm + q]); sg.push_back(1); }
    const size_t nA = lst.size();
    for (int q = 0; q < ntp; q++) { lst.push_back(tab[o_tc + q]); sg.push_back(1); }
    const size_t nBs = lst.size() - nA;
    for (int q = 0; q < 2 * ncp; q++) { lst.push_back(tab[ncp + q]); sg.push_back(-1); }
    for (int q = 0; q < ntp; q++) { lst.push_back(tab[o_tx + q]); sg.push_back(-1); }
    for (int q = 0; q < ntp; q++) { lst.push_back(tab[o_ty + q]); sg.push_back(-1); }
    const size_t nBv = lst.size() - nA - nBs, nall = nplanes + lst.size();
    HIPCHK(c, grow(c, c->rm_tab, c->rm_tab_n, nall));
    HIPCHK(c, grow(c, c->rm_sgn, c->rm_sgn_n, nall));
    HIPCHK(c, hipMemcpyAsync(c->rm_tab, tab.data(), sizeof(double *) * nplanes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rm_tab + nplanes, lst.data(), sizeof(double *) * lst.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rm_sgn, sg.data(), sg.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rm_bad, 0, sizeof(unsigned), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (tab, lst, sg are pageable host vectors)
    RemapPlanes P{(double *const *)c->rm_tab, ncp, ntp};
    // the caller's arrays: in place where their memory is visible to the device, else through a staging copy
    const size_t n_mm = (size_t)c->nblocks * ncp * nblk, n_tm = (size_t)c->nblocks * ntp * nblk;
    const dim3 b(64, 4);
    const int nrg = (c->nyb + 3) / 4;
    if ((long long)nrg * c->nblocks > 65535 || ntp > 65535) FAIL(c, "evpk_transport_remap: too many blocks for one launch");
    double *dmm = nullptr, *dtm = nullptr;
    RemapState io{};
    std::vector<HostArr> arr;
    if (!st) {
        arr = {{mm, n_mm, &dmm, true}, {tm, n_tm, &dtm, true}};
        if (stage_in(c, arr)) return 1;
        // mm(nx_block, ny_block, 0:ncat, max_blocks), tm(nx_block, ny_block, ntrace, ncat, max_blocks) -> planes, one launch per array
        hipLaunchKernelGGL(k_gather_planes, dim3((c->nxb + 63) / 64, nrg * c->nblocks, ncp), b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)dmm,
                           nblk, (size_t)ncp * nblk, (double *const *)c->rm_tab, nrg);
        if (ntp)
            hipLaunchKernelGGL(k_gather_planes, dim3((c->nxb + 63) / 64, nrg * c->nblocks, ntp), b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, (const double *)dtm,
                               nblk, (size_t)ntp * nblk, (double *const *)(c->rm_tab + o_tm), nrg);
    } else {
        // aice0, aicen, vicen, vsnon, trcrn: state_to_tracers inside the gather
        io = *st;
        const size_t N = (size_t)c->nblocks * nblk;
        arr = {{st->aice0, N, &io.aice0, true}, {st->aicen, N * ncat, &io.aicen, true}, {st->vicen, N * ncat, &io.vicen, true},
               {st->vsnon, N * ncat, &io.vsnon, true}, {st->trcrn, N * ncat * st->ntrcr_dim, &io.trcrn, true}};
        if (stage_in(c, arr)) return 1;
        hipLaunchKernelGGL(k_state_gather, dim3((c->nxb + 63) / 64, nrg * c->nblocks, ncp), b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, io, P, nrg);
    }
    HIPCHK(c, hipGetLastError());
    double **dl = c->rm_tab + nplanes;
    if (planes_halo(c, dl, c->rm_sgn, (int)nA, false)) return 1;
    const double *dxu = c->rm_grid, *dyu = c->rm_grid + np, *hm = c->rm_grid + 2 * np;
    const dim3 g2 = grid2d(s, B2D);
    hipLaunchKernelGGL(k_remap_construct, dim3(g2.x, g2.y, ncp), B2D, 0, c->stream, s, tb, P, hm);
    if (planes_halo(c, dl + nA, c->rm_sgn + nA, (int)nBs, false)) return 1;
    if (planes_halo(c, dl + nA + nBs, c->rm_sgn + nA + nBs, (int)nBv, true)) return 1;
    // departure points in the sig1 / sig2 planes (scratch between calls of evpk_principal_stress), NE-corner vectors (:564-570)
    const int SB = c->cur ? F_STATE1 : F_STATE0;
    hipLaunchKernelGGL(k_remap_dp, g2, B2D, 0, c->stream, s, SB, dt, dxu, dyu, tb.midpt, (int)F_SIG1, (int)F_SIG2, c->rm_bad);
    if (halo(c, F_SIG1, 2, true, true, 0.0)) return 1;
    // fluxes + update: one tiled kernel whose edge transports stay in the LDS (EVPK_REMAP_FUSED=0 or more than 14 tracers: the
    // three kernels that hand fe, fn, tfe, tfn over through HBM)
    bool remap_direct = false;
    const size_t flux_lds = sizeof(double) * 2 * 256 * (size_t)(1 + ntrace);
    if (env_on("EVPK_REMAP_FUSED") && flux_lds <= 60 * 1024) {
        const long long ntiles = (long long)((s.nxl + RM_TILE - 2) / (RM_TILE - 1)) * ((s.nyl + RM_TILE - 2) / (RM_TILE - 1)) * ncp;
        // without the state transforms the update delivers straight into the caller's arrays (device-visible, or the staged copy
        // that is sent back below): no scatter pass.  A bad departure point leaves them untouched (the kernel looks at the flag
        // k_remap_dp set); a negative mass is found while they are being written -- the reference aborts the run there
        // (:3622-3640), the arrays are then undefined (include/evpk.h).  EVPK_REMAP_DIRECT=0: planes + scatter as before.
        remap_direct = !st && env_on("EVPK_REMAP_DIRECT");
        RmOut O{};
        if (remap_direct) {
            if (remap_block_map(c)) return 1;
            O.mm = dmm; O.tm = dtm; O.bmap = c->d_bmap; O.bd = c->d_bd; O.direct = 1; O.nbxg = c->bmap_nbx; O.bsx = c->nxb - 2; O.bsy = c->nyb - 2;
            O.nxb = c->nxb; O.nyb = c->nyb;
        }
        hipLaunchKernelGGL(k_remap_fluxupd, dim3((unsigned)(((ntiles + 7) / 8) * 8)), dim3(256), flux_lds, c->stream,
                           s, tb, P, dxu, dyu, (int)F_SIG1, (int)F_SIG2, c->rm_bad, O);
        // the new masses were written beside the old ones (plane fe(n)): in place of mm(n) now that every tile is done
        if (!remap_direct)
            HIPCHK(c, hipMemcpyAsync(c->rm_pool, c->rm_pool + (size_t)3 * ncp * np, sizeof(double) * (size_t)ncp * np, hipMemcpyDeviceToDevice, c->stream));
    } else {
    hipLaunchKernelGGL(k_remap_flux<false>, dim3((s.nxl + 1 + 63) / 64, (s.nyl + 3) / 4, ncp), B2D, 0, c->stream, s, tb, P, dxu, dyu, (int)F_SIG1, (int)F_SIG2);
    hipLaunchKernelGGL(k_remap_flux<true>, dim3((s.nxl + 63) / 64, (s.nyl + 1 + 3) / 4, ncp), B2D, 0, c->stream, s, tb, P, dxu, dyu, (int)F_SIG1, (int)F_SIG2);
    hipLaunchKernelGGL(k_remap_update, dim3((s.nxl + 63) / 64, (s.nyl + 3) / 4, ncp), B2D, 0, c->stream, s, tb, P, c->rm_bad);
    }
    HIPCHK(c, hipGetLastError());
    unsigned bad = 0;
    HIPCHK(c, hipMemcpyAsync(&bad, c->rm_bad, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (xp_check(c)) return 1;
    // Ranks decide alone, as the reference's l_stop is per task (the caller aborts the run, abort_ice) -- but a rank that
    // found a bad cell still takes part in the one exchange left on the state path (bound_state's ghost-ring update below),
    // so that its slab neighbours are not left waiting for a partner: they return normally, it returns the error afterwards.
    int badrc = 0;
    if (bad & 1u) { c->err = "evpk_transport_remap: departure points out of bounds (ice_transport_remap.F90:1583-1607)"; badrc = EVPK_REMAP_BAD_DEPARTURE; }
    else if (bad & 2u) { c->err = "evpk_transport_remap: negative area / mass after the update (ice_transport_remap.F90:3622-3640)"; badrc = EVPK_REMAP_NEGATIVE_MASS; }
    if (badrc && !(st && c->nranks > 1)) return badrc;
    if (!st) {
        if (!remap_direct) {
        hipLaunchKernelGGL(k_scatter_planes, dim3((c->nxb + 63) / 64, nrg * c->nblocks, ncp), b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb,
                           (double *const *)c->rm_tab, dmm, nblk, (size_t)ncp * nblk, nrg);
        if (ntp)
            hipLaunchKernelGGL(k_scatter_planes, dim3((c->nxb + 63) / 64, nrg * c->nblocks, ntp), b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb,
                               (double *const *)(c->rm_tab + o_tm), dtm, nblk, (size_t)ntp * nblk, nrg);
        }
        HIPCHK(c, hipGetLastError());
    } else {
        // bound_state: the ghost ring of the NEW areas and tracers, then tracers_to_state on every cell of every block
        if (planes_halo(c, dl, c->rm_sgn, (int)nA, false)) return 1;
        if (badrc) {                                  // the caller's arrays stay untouched
            const std::string keep = c->err;
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (xp_check(c)) return 1;
            c->err = keep;
            return badrc;
        }
        hipLaunchKernelGGL(k_state_scatter, dim3((c->nxb + 63) / 64, nrg * c->nblocks, ncp), b, 0, c->stream, s, c->d_bd, c->nxb, c->nyb, io, P, nrg);
        HIPCHK(c, hipGetLastError());
    }
    return stage_out(c, arr);
}

extern "C" int evpk_transport_remap(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrace, double *mm, double *tm, const int32_t *tracer_type,
                                    const int32_t *depend, const int32_t *has_dependents, int32_t integral_order, int32_t l_dp_midpt,
                                    int32_t l_fixed_area) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    return remap_impl(c, dt, ncat, ntrace, mm, tm, tracer_type, depend, has_dependents, integral_order, l_dp_midpt, l_fixed_area, nullptr);
}

extern "C" int evpk_transport_remap_state(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, int32_t nt_qsno, int32_t nslyr,
                                          double rhos_lfresh, double *aice0, double *aicen, double *vicen, double *vsnon, double *trcrn,
                                          const int32_t *tracer_type, const int32_t *depend, const int32_t *has_dependents,
                                          int32_t integral_order, int32_t l_dp_midpt) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c || !aice0 || !aicen || !vicen || !vsnon || ntrcr < 0 || (ntrcr > 0 && !trcrn) || ntrcr_dim < ntrcr) return 1;
    RemapState st{};
    st.aice0 = aice0; st.aicen = aicen; st.vicen = vicen; st.vsnon = vsnon; st.trcrn = trcrn;
    st.ncat = ncat; st.ntrcr = ntrcr; st.ntrcr_dim = ntrcr_dim; st.nt_qsno = nt_qsno; st.nslyr = nslyr; st.shift = rhos_lfresh;
    return remap_impl(c, dt, ncat, 2 + ntrcr, nullptr, nullptr, tracer_type, depend, has_dependents, integral_order, l_dp_midpt, 0, &st);
}

// ---- step_dynamics behind evp / eap (source/ice_step_mod.F90:1126-1192) in one call ----
// the four entry points in the reference's order on the arrays of x; a stop fills stop[0] with the stage and stop[1..4] with its numbers
static int dyn_stages(evpk_ctx *c, const evpk_dyn_args &x, evpk_ridge_diag *dg, int32_t stop[5]) {
    const evpk_itd_tracers &t = x.t;
    int32_t s4[4] = {0, 0, 0, 0};
    int rc = 0;
    // Ranks decide alone, as the reference's l_stop is per task -- but a rank whose stage stops still posts the exchange of the call
    // that is left, aggregate's bound_state, with whatever its arrays hold, so that its slab neighbours are not left waiting: they
    // return normally, it returns its stage's code afterwards (include/evpk.h)
    auto stopped = [&](int code) {
        if (c->nranks == 1 || c->check_only || code == 1) return code;
        const std::string keep = c->err;
        ItdArgs A{};
        A.ncat = x.ncat; A.ntrcr = x.ntrcr; A.ntrcr_dim = x.ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb;
        A.aicen = x.aicen; A.vicen = x.vicen; A.vsnon = x.vsnon; A.trcrn = x.ntrcr ? x.trcrn : nullptr;
        if (itd_bound(c, A, "evpk_step_dynamics") || hipStreamSynchronize(c->stream) != hipSuccess || xp_check(c)) return 1;
        c->err = keep;
        return code;
    };
    if (x.advection == 1)
        rc = evpk_transport_upwind_state(c, x.dt, x.ncat, x.ntrcr, x.ntrcr_dim, x.trcr_depend, t.nt_Tsfc, t.nt_alvl, t.nt_apnd, t.nt_fbri, t.tr_pond_cesm,
                                         t.tr_pond_lvl, t.tr_pond_topo, x.k.Tocnfrz, x.aice0, x.aicen, x.vicen, x.vsnon, x.trcrn);
    else if (x.advection == 2)
        rc = evpk_transport_remap_state(c, x.dt, x.ncat, x.ntrcr, x.ntrcr_dim, t.nt_qsno, t.nslyr, x.rhos_lfresh, x.aice0, x.aicen, x.vicen, x.vsnon,
                                        x.trcrn, x.tracer_type, x.depend, x.has_dependents, x.integral_order, x.l_dp_midpt);
    if (rc) {
        if (rc == EVPK_REMAP_BAD_DEPARTURE || rc == EVPK_REMAP_NEGATIVE_MASS) stop[0] = 1;
        return stopped(rc);
    }
    if (x.ridge) {
        const evpk_ridge_tracers rt{t.nt_qsno, t.nslyr, t.nt_alvl, x.nt_vlvl, t.nt_apnd, t.nt_hpnd, t.nt_fbri, t.tr_pond_cesm, t.tr_pond_lvl, t.tr_pond_topo};
        rc = evpk_ridge_ice(c, x.dt, x.ndtd, x.ncat, x.ntrcr, x.ntrcr_dim, x.trcr_depend, &rt, x.hin_max, x.rdg_conv, x.rdg_shear, x.aice0, x.aicen,
                            x.vicen, x.vsnon, x.trcrn, dg, s4);
        if (rc) {
            if (rc == EVPK_RIDGE_STOP) { stop[0] = 2; for (int q = 0; q < 4; q++) stop[1 + q] = s4[q]; }
            return stopped(rc);
        }
    }
    rc = evpk_cleanup_itd(c, x.dt * x.ndtd, x.ncat, x.ntrcr, x.ntrcr_dim, x.trcr_depend, &t, x.hin_max, &x.k, x.tr_aero, x.nbtrcr, x.heat_capacity,
                          x.aicen, x.vicen, x.vsnon, x.trcrn, x.aice0, x.aice, x.fpond, x.fresh, x.fsalt, x.fhocn, x.first_ice, s4);
    if (rc) {
        if (rc == EVPK_ITD_STOP) { stop[0] = 3; for (int q = 0; q < 4; q++) stop[1 + q] = s4[q]; }
        return stopped(rc);
    }
    return evpk_aggregate(c, x.dt, 1, x.ncat, x.ntrcr, x.ntrcr_dim, x.trcr_depend, &t, x.nt_iage, x.k.Tocnfrz, x.aicen, x.vicen, x.vsnon, x.trcrn,
                          x.aice, x.vice, x.vsno, x.aice0, x.trcr, x.daidtd, x.dvidtd, x.dagedtd);
}

extern "C" int evpk_step_dynamics(evpk_ctx *c, const evpk_dyn_args *a, int32_t stop[5]) {
    if (!c) return 1;
    if (stop) stop[0] = stop[1] = stop[2] = stop[3] = stop[4] = 0;
    RANKS_ENTRY(c, "evpk_step_dynamics");
    if (!a || !stop) FAIL(c, "evpk_step_dynamics: a required argument is missing");
    if (a->advection < 0 || a->advection > 2) FAIL(c, "evpk_step_dynamics: advection = %d not in 0..2", a->advection);
    if (a->ridge != 0 && a->ridge != 1) FAIL(c, "evpk_step_dynamics: ridge = %d", a->ridge);
    if (!a->hin_max || !a->aice0 || !a->aicen || !a->vicen || !a->vsnon || !a->aice || !a->vice || !a->vsno || a->ntrcr < 0 || a->ntrcr_dim < a->ntrcr ||
        (a->ntrcr > 0 && (!a->trcrn || !a->trcr || !a->trcr_depend)))
        FAIL(c, "evpk_step_dynamics: a required argument is missing");
    if (!(a->dt > 0.0) || a->ndtd < 1) FAIL(c, "evpk_step_dynamics: dt = %g, ndtd = %d", a->dt, a->ndtd);
    if (a->ncat < 1 || a->ncat > MAXCAT) FAIL(c, "evpk_step_dynamics: ncat = %d not in 1..%d", a->ncat, MAXCAT);
    if (!c->connected) FAIL(c, "evpk_step_dynamics: the context is not connected yet (evpk_connect)");
    evpk_ridge_diag dg{};
    if (a->diag) dg = *a->diag;
    dg.fpond = a->fpond; dg.fresh = a->fresh; dg.fhocn = a->fhocn;
    // what the stages refuse, before the first copy: each of them with the caller's own pointers, returning after its checks
    {
        int32_t s5[5] = {0, 0, 0, 0, 0};
        c->check_only = true;
        const int rc = dyn_stages(c, *a, &dg, s5);
        c->check_only = false;
        if (rc) return rc;
    }
    if (!c->nblocks && c->nranks == 1) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    // the union of the caller's arrays, each staged once (or used in place): the stages then see device pointers only
    evpk_dyn_args x = *a;
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb, n3 = N * a->ncat;
    const bool tr = a->ntrcr > 0;
    std::vector<HostArr> arr = {
        {a->aice0, N, &x.aice0, true}, {a->aicen, n3, &x.aicen, true}, {a->vicen, n3, &x.vicen, true}, {a->vsnon, n3, &x.vsnon, true},
        {tr ? a->trcrn : nullptr, n3 * a->ntrcr_dim, &x.trcrn, true}, {a->aice, N, &x.aice, true}, {a->vice, N, &x.vice, true},
        {a->vsno, N, &x.vsno, true}, {tr ? a->trcr : nullptr, N * a->ntrcr_dim, &x.trcr, true}, {a->daidtd, N, &x.daidtd, true},
        {a->dvidtd, N, &x.dvidtd, true}, {a->dagedtd, N, &x.dagedtd, true}, {a->fpond, N, &x.fpond, true}, {a->fresh, N, &x.fresh, true},
        {a->fsalt, N, &x.fsalt, true}, {a->fhocn, N, &x.fhocn, true}, {a->first_ice, n3, &x.first_ice, true}};
    if (a->ridge) {         // (the rates and the diagnostics belong to ridge_ice alone)
        arr.push_back({a->rdg_conv, N, &x.rdg_conv, false}); arr.push_back({a->rdg_shear, N, &x.rdg_shear, false});
        for (double **p : {&dg.dardg1dt, &dg.dardg2dt, &dg.dvirdgdt, &dg.opening}) arr.push_back({*p, N, p, true});
        for (double **p : {&dg.dardg1ndt, &dg.dardg2ndt, &dg.dvirdgndt, &dg.aparticn, &dg.krdgn, &dg.araftn, &dg.vraftn, &dg.aredistn, &dg.vredistn})
            arr.push_back({*p, n3, p, true});
    }
    if (stage_in(c, arr, true)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    dg.fpond = x.fpond; dg.fresh = x.fresh; dg.fhocn = x.fhocn;
    const int rc = dyn_stages(c, x, &dg, stop);
    if (rc == 1) return 1;
    const std::string keep = c->err;
    if (stage_out(c, arr)) return 1;
    if (rc) c->err = keep;
    return rc;
}

// ---- step_therm2 (source/ice_step_mod.F90:741-995) in one call: the frain line, aggregate_area, linear_itd, add_new_ice with
// lateral_melt (kernels in evpk_therm2.hip), cleanup_itd ----
// what both entry points refuse, and the kernel arguments of one call on the pointers of x (the caller's own, or device pointers)
static int therm2_args(evpk_ctx *c, const char *who, const evpk_therm2_args &x, ItdArgs &A, Therm2Args &T) {
    const evpk_itd_tracers &t = x.t;
    if (t.tr_brine || x.skl_bgc) FAIL(c, "%s: tr_brine / skl_bgc (add_new_ice_bgc) are not supported", who);
    if (x.tr_aero) FAIL(c, "%s: aerosol tracers (tr_aero) are not supported: faero_ocn cannot be passed", who);
    if (x.nbtrcr > 0) FAIL(c, "%s: nbtrcr = %d: bgc tracers are not supported: flux_bio cannot be passed", who, x.nbtrcr);
    if (!x.heat_capacity) FAIL(c, "%s: heat_capacity = .false. is not supported", who);
    if (x.ktherm != 1 && x.ktherm != 2) FAIL(c, "%s: ktherm = %d not 1 or 2", who, x.ktherm);
    if (x.kitd != 0 && x.kitd != 1) FAIL(c, "%s: kitd = %d not 0 or 1", who, x.kitd);
    if (!x.hin_max || !x.aicen_init || !x.vicen_init || !x.aicen || !x.vicen || !x.vsnon || !x.aice || !x.aice0 || !x.frzmlt || !x.Tf || !x.sss ||
        !x.rside || !x.salinz || !x.frazil || !x.meltl || !x.fresh || !x.fsalt || !x.fhocn || x.ntrcr < 0 || x.ntrcr_dim < x.ntrcr ||
        (x.ntrcr > 0 && (!x.trcrn || !x.trcr_depend)))
        FAIL(c, "%s: a required argument is missing", who);
    if (!c->connected) FAIL(c, "%s: the context is not connected yet (evpk_connect)", who);
    if (!c->have_params) FAIL(c, "%s: evpk_set_params has not been called (rhow, rhoi, rhos)", who);
    if (!(x.dt > 0.0)) FAIL(c, "%s: dt = %g", who, x.dt);
    if (x.ncat < 1 || x.ncat > MAXCAT) FAIL(c, "%s: ncat = %d not in 1..%d", who, x.ncat, MAXCAT);
    if (x.ntrcr > RG_MAXT) FAIL(c, "%s: ntrcr = %d exceeds %d", who, x.ntrcr, RG_MAXT);
    if (x.k.puny != 1.0e-11) FAIL(c, "%s: puny = %g: compute_tracers on the device is built with 1e-11", who, x.k.puny);
    if (tracer_tables(c, who, A, x.ntrcr, x.trcr_depend, t, x.nt_vlvl)) return 1;
    if (x.ntrcr > 0 && (t.nt_Tsfc < 1 || t.nt_qice < 1 || x.nt_sice < 1)) FAIL(c, "%s: nt_Tsfc, nt_qice and nt_sice are required", who);
    if (t.nilyr > T2_MAXL || t.nslyr > T2_MAXL) FAIL(c, "%s: nilyr = %d, nslyr = %d exceed %d", who, t.nilyr, t.nslyr, T2_MAXL);
    if (x.ntrcr > 0 && x.nt_sice + t.nilyr - 1 > x.ntrcr) FAIL(c, "%s: nt_sice / nilyr beyond ntrcr", who);
    for (int q : {x.nt_iage, x.nt_FY, x.nt_vlvl}) if (q < 0 || q > x.ntrcr) FAIL(c, "%s: tracer index %d not in 0..ntrcr = %d", who, q, x.ntrcr);
    if ((t.tr_pond_cesm || t.tr_pond_lvl) && t.nt_apnd < 1) FAIL(c, "%s: ponds without nt_apnd", who);
    if (t.tr_pond_lvl && (t.nt_alvl < 1 || x.nt_vlvl < 1)) FAIL(c, "%s: tr_pond_lvl without nt_alvl / nt_vlvl", who);
    if (t.tr_pond_topo && !x.fpond) FAIL(c, "%s: tr_pond_topo needs fpond", who);
    A.nt_Tsfc = t.nt_Tsfc; A.nt_qice = t.nt_qice; A.nilyr = x.ntrcr ? t.nilyr : 0; A.nt_qsno = t.nt_qsno; A.nslyr = x.ntrcr ? t.nslyr : 0;
    A.nt_alvl = t.nt_alvl; A.nt_apnd = t.nt_apnd; A.nt_hpnd = t.nt_hpnd; A.tr_pond_topo = t.tr_pond_topo ? 1 : 0;
    A.ncat = x.ncat; A.ntrcr = x.ntrcr; A.ntrcr_dim = x.ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb;
    A.dt = x.dt; A.salinity = x.k.ice_ref_salinity; A.cp_ice = x.k.cp_ice; A.Lfresh = x.k.Lfresh; A.puny = x.k.puny; A.rhoi = c->p.rhoi;
    A.rhos = c->p.rhos;
    A.hin_max[0] = x.hin_max[0];
    A.aicen = x.aicen; A.vicen = x.vicen; A.vsnon = x.vsnon; A.trcrn = x.ntrcr ? x.trcrn : nullptr; A.aice = x.aice; A.aice0 = x.aice0;
    A.fpond = t.tr_pond_topo ? x.fpond : nullptr; A.fresh = x.fresh; A.fsalt = x.fsalt; A.fhocn = x.fhocn;
    T.aicen_init = x.aicen_init; T.vicen_init = x.vicen_init; T.frain = x.frain; T.frzmlt = x.frzmlt; T.Tf = x.Tf; T.sss = x.sss; T.rside = x.rside;
    T.salinz = x.salinz; T.frazil = x.frazil; T.frz_onset = x.frz_onset; T.meltl = x.meltl;
    T.ktherm = x.ktherm; T.update_ocn_f = x.update_ocn_f ? 1 : 0; T.nt_sice = x.nt_sice; T.nt_iage = x.nt_iage; T.nt_FY = x.nt_FY;
    T.nt_vlvl = x.nt_vlvl; T.tr_pond_cesm = t.tr_pond_cesm ? 1 : 0; T.tr_pond_lvl = t.tr_pond_lvl ? 1 : 0;
    T.yday = x.yday; T.hfrazilmin = x.hfrazilmin; T.phi_init = x.phi_init; T.dSin0_frazil = x.dSin0_frazil; T.cp_ocn = x.cp_ocn; T.rhow = c->p.rhow;
    T.hi0max = x.ncat > 1 ? x.hin_max[1] * 0.9 : 1.0e30;  // ice_therm_itd.F90:1416-1420 (bignum)
    return 0;
}

// the caller's arrays of section 1 (and of the stages around it when `step`), each staged once or used in place
static std::vector<HostArr> therm2_arrays(evpk_ctx *c, const evpk_therm2_args &a, evpk_therm2_args &x, bool step) {
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb, n3 = N * a.ncat;
    const bool tr = a.ntrcr > 0;
    std::vector<HostArr> arr = {
        {a.aicen_init, n3, &x.aicen_init, false}, {a.vicen_init, n3, &x.vicen_init, false},
        {a.aicen, n3, &x.aicen, true}, {a.vicen, n3, &x.vicen, true}, {a.vsnon, n3, &x.vsnon, true},
        {tr ? a.trcrn : nullptr, n3 * a.ntrcr_dim, &x.trcrn, true}, {a.aice, N, &x.aice, step}, {a.aice0, N, &x.aice0, true},
        {a.frzmlt, N, &x.frzmlt, false}, {a.Tf, N, &x.Tf, false}, {a.sss, N, &x.sss, false}, {a.rside, N, &x.rside, false},
        {a.salinz, N * (a.t.nilyr + 1), &x.salinz, false}, {a.frazil, N, &x.frazil, true}, {a.frz_onset, N, &x.frz_onset, true},
        {a.meltl, N, &x.meltl, true}, {(a.t.tr_pond_topo || step) ? a.fpond : nullptr, N, &x.fpond, true}, {a.fresh, N, &x.fresh, true},
        {a.fsalt, N, &x.fsalt, true}, {a.fhocn, N, &x.fhocn, true}};
    if (step) {
        arr.push_back({a.frain, N, &x.frain, false});
        arr.push_back({a.first_ice, n3, &x.first_ice, true});
    }
    return arr;
}

extern "C" int evpk_new_ice_lateral_melt(evpk_ctx *c, const evpk_therm2_args *a) {
    if (!c) return 1;
    RANKS_ENTRY(c, "evpk_new_ice_lateral_melt");
    if (!a) FAIL(c, "evpk_new_ice_lateral_melt: a required argument is missing");
    ItdArgs A{};
    Therm2Args T{};
    if (therm2_args(c, "evpk_new_ice_lateral_melt", *a, A, T)) return 1;
    if (!c->nblocks || c->check_only) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    evpk_therm2_args x = *a;
    std::vector<HostArr> arr = therm2_arrays(c, *a, x, false);
    if (stage_in(c, arr)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    if (therm2_args(c, "evpk_new_ice_lateral_melt", x, A, T)) return 1;
    const dim3 b(64), g = block_grid(c);
    if (a->ncat == 5 && A.nilyr == 4)
        hipLaunchKernelGGL((k_therm2_leads<5, 4>), g, b, 0, c->stream, c->s, (const BlockDesc *)c->d_bd, A, T);
    else
        hipLaunchKernelGGL((k_therm2_leads<0, 0>), g, b, 0, c->stream, c->s, (const BlockDesc *)c->d_bd, A, T);
    HIPCHK(c, hipGetLastError());
    return stage_out(c, arr);
}

// the stages of evpk_step_therm2 on the arrays of x; a stop fills stop[0] with the stage and stop[1..4] with its numbers
static int therm2_stages(evpk_ctx *c, const evpk_therm2_args &x, int32_t stop[5]) {
    int32_t s4[4] = {0, 0, 0, 0};
    if (!c->check_only && c->nblocks) {                   // the frain line and aggregate_area on every cell
        ItdArgs A{};
        Therm2Args T{};
        if (therm2_args(c, "evpk_step_therm2", x, A, T)) return 1;
        with_ncat(x.ncat, [&](auto NC) {
            constexpr int nc = decltype(NC)::value;
            hipLaunchKernelGGL(k_therm2_open<nc>, block_grid(c), dim3(64), 0, c->stream, A, T.frain);
        });
        HIPCHK(c, hipGetLastError());
    }
    int rc = 0;
    if (x.kitd == 1) {
        rc = evpk_linear_itd(c, x.ncat, x.ntrcr, x.ntrcr_dim, x.trcr_depend, &x.t, x.hin_max, x.hi_min, &x.k, x.aicen_init, x.vicen_init, x.aicen,
                             x.vicen, x.vsnon, x.trcrn, x.aice, x.aice0, x.fpond, s4);
        if (rc) {
            if (rc == EVPK_LITD_STOP) { stop[0] = 1; for (int q = 0; q < 4; q++) stop[1 + q] = s4[q]; }
            return rc;
        }
    }
    rc = evpk_new_ice_lateral_melt(c, &x);
    if (rc) return rc;
    rc = evpk_cleanup_itd(c, x.dt, x.ncat, x.ntrcr, x.ntrcr_dim, x.trcr_depend, &x.t, x.hin_max, &x.k, x.tr_aero, x.nbtrcr, x.heat_capacity, x.aicen,
                          x.vicen, x.vsnon, x.trcrn, x.aice0, x.aice, x.fpond, x.fresh, x.fsalt, x.fhocn, x.first_ice, s4);
    if (rc == EVPK_ITD_STOP) { stop[0] = 3; for (int q = 0; q < 4; q++) stop[1 + q] = s4[q]; }
    return rc;
}

extern "C" int evpk_step_therm2(evpk_ctx *c, const evpk_therm2_args *a, int32_t stop[5]) {
    if (!c) return 1;
    if (stop) stop[0] = stop[1] = stop[2] = stop[3] = stop[4] = 0;
    RANKS_ENTRY(c, "evpk_step_therm2");
    if (!a || !stop) FAIL(c, "evpk_step_therm2: a required argument is missing");
    {       // what the stages refuse, before the first copy: each of them with the caller's own pointers, returning after its checks
        ItdArgs A{};
        Therm2Args T{};
        if (therm2_args(c, "evpk_step_therm2", *a, A, T)) return 1;
        int32_t s5[5] = {0, 0, 0, 0, 0};
        c->check_only = true;
        const int rc = therm2_stages(c, *a, s5);
        c->check_only = false;
        if (rc) return rc;
    }
    if (!c->nblocks) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    evpk_therm2_args x = *a;
    std::vector<HostArr> arr = therm2_arrays(c, *a, x, true);
    if (stage_in(c, arr, true)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    const int rc = therm2_stages(c, x, stop);
    if (rc == 1) return 1;
    const std::string keep = c->err;
    if (stage_out(c, arr)) return 1;
    if (rc) c->err = keep;
    return rc;
}

// ---- the column physics behind step_therm2: thermo_vertical, step_therm1, step_radiation (ccsm3, dEdd), prep_radiation ----
#include "evpk_api_column.hip"

extern "C" int evpk_calibrate(evpk_ctx *c, int32_t nrep) {
    if (c && c->idle) return 0;       // a rank without a block column: in no exchange, nothing to compute
    if (!c) return 1;
    HIPCHK(c, hipSetDevice(c->device));
    for (int n = 0; n < nrep; n++)   // WORK1/WORK2 pair plane: scratch, rewritten by the next prep/finish
        hipLaunchKernelGGL(k_calib_copy_pair, grid2d(c->s, B2D), B2D, 0, c->stream, c->s, (int)(F_WORK1 & ~1), (int)(F_WORK1 & ~1));   // in place: same bytes read and written
    HIPCHK(c, hipGetLastError());
    // ... and EVPK_CALIB_BIG_BYTES (1 GiB) each way between two buffers of their own: four times the Infinity Cache, so that
    // neither the reads nor the writes can be served on the die (MI355X_MICROARCH.md, Infinity Cache)
    double2 *a = nullptr, *b = nullptr;
    const size_t n = EVPK_CALIB_BIG_BYTES / sizeof(double2);
    HIPCHK(c, hipMalloc(&a, EVPK_CALIB_BIG_BYTES));
    if (hipMalloc(&b, EVPK_CALIB_BIG_BYTES) != hipSuccess) { (void)hipFree(a); FAIL(c, "evpk_calibrate: hipMalloc failed"); }
    (void)hipMemsetAsync(a, 0x11, EVPK_CALIB_BIG_BYTES, c->stream);
    (void)hipMemsetAsync(b, 0x22, EVPK_CALIB_BIG_BYTES, c->stream);
    for (int k = 0; k < nrep; k++)
        hipLaunchKernelGGL(k_calib_copy_big, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double2 *)a, b, n);
    for (int k = 0; k < nrep; k++)      // ... and with 8 B per lane: the plain planes of rows f-3 / f-4
        hipLaunchKernelGGL(k_calib_copy_big8, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, c->stream, (const double *)a, (double *)b, 2 * n);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
    (void)hipFree(a); (void)hipFree(b);
    if (e1 != hipSuccess || e2 != hipSuccess) FAIL(c, "evpk_calibrate: copy failed");
    return 0;
}

extern "C" int evpk_get_stats(evpk_ctx *c, evpk_stats *o) {
    if (!c || !o) return 1;
    if (c->counts_pending) {      // between evpk_prep and the first evpk_subcycle on the device-compacted path: wait for the counts
        if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) FAIL(c, "evpk_get_stats: hipStreamSynchronize failed");
        take_counts(c);
        if (xp_check(c)) return 1;    // (evpk_prep's own exchanges on this path are only checked here or after the loop)
    }
    o->icellt = c->icellt; o->icellu = c->icellu;
    o->ncell_slab = (int64_t)c->s.nxl * c->s.nyl;
    o->nstrips = c->nstrips; o->nstrips_total = c->ncx * c->nry;
    o->subcycles_done = c->ksub;
    o->loop_ms = c->loop_ms;
    o->kernel_ms = c->kernel_ms; o->kernel_launches = c->kernel_launches - c->double_launches;
    o->kernel2_ms = c->kernel2_ms; o->kernel2_launches = c->double_launches;
    o->strip_rows = c->R; o->strip_rows2 = c->use_double ? c->R2 : 0; o->nstrips2 = c->use_double ? c->nstrips2 : 0;
    o->zone_cols = c->zone_mode ? c->zW : 0; o->zone_exchanges = c->zone_exchanges; o->zone_bytes = c->zone_bytes;
    o->overlap_split = !c->ov_fixed ? -1 : (c->overlap ? 1 : 0);
    o->tile_kernel = (c->use_double && c->tile_mode) ? 1 : 0;
    o->kernel_timed = c->kernel_timed; o->kernel2_timed = c->kernel2_timed;
    o->bound_ms = c->bound_ms; o->bound_updates = c->bound_updates;
    o->compact_metrics = c->compact ? 1 : 0;
    o->transport = c->ipc ? EVPK_XP_IPC : c->relay ? EVPK_XP_SHM_RELAY : (c->xranks > 1 ? EVPK_XP_RCCL : (c->comm ? EVPK_XP_RCCL : (c->force_exchange ? EVPK_XP_SELF : EVPK_XP_NONE)));
    o->band_row_exchanges = c->xb_swaps;
    o->kernel3_ms = 0.f; o->kernel3_launches = 0; o->kernel3_timed = 0;      // reserved, always 0 (read by bench.py)
    o->strip_rows3 = 0; o->nstrips3 = 0;
    int nr = 0;
    if (c->comm && ncclCommCount(c->comm, &nr) != ncclSuccess) nr = -1;
    o->rccl_ranks = nr;
    o->device = c->device;
    int dom = 0, bus = 0, dev = 0;
    (void)hipDeviceGetAttribute(&dom, hipDeviceAttributePciDomainID, c->device);
    (void)hipDeviceGetAttribute(&bus, hipDeviceAttributePciBusId, c->device);
    (void)hipDeviceGetAttribute(&dev, hipDeviceAttributePciDeviceId, c->device);
    o->device_pci = (dom << 16) | (bus << 8) | dev;
    o->delivery_checked = c->dv_checked; o->delivery_bad = c->dv_bad;
    o->bound_state_rounds = c->bs_rounds; o->bound_state_planes = c->bs_planes;
    return 0;
}
