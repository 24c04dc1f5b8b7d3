/*
 * evpk.h -- C ABI of the MI355X EVP sea-ice dynamics solver (libevpk.so).
 *
 * This is the drop-in boundary for ONE path of COSIMA/cice5: the body of
 *     subroutine evp(dt)                      source/ice_dyn_evp.F90:68-510
 * i.e. evp_prep1/evp_prep2 (source/ice_dyn_shared.F90:270,377), the ndte-subcycled
 * stress + stepu loop with its velocity halo update (ice_dyn_evp.F90:336-410,
 * :520-849; ice_dyn_shared.F90:623-748), the tripole stress fold (:416-481),
 * evp_finish (ice_dyn_shared.F90:757) and the T<->U averages around them
 * (source/ice_grid.F90:1799-1958).  The reference has no FFI for this path: the
 * boundary there is a Fortran module procedure plus module-global arrays
 * (SURVEY.md S8b).  The entry points below are what a Fortran `ice_dyn_evp`
 * replacement binds through ISO_C_BINDING (fortran/evpk_mod.F90, fortran/ice_dyn_evp.F90,
 * INTEGRATION.md).
 *
 * Conventions
 *  - plain C, no C++/torch types; every array is a caller-owned host buffer borrowed for
 *    the duration of the call only.
 *  - every field is the reference's block array  real(8) a(nx_block,ny_block,nblocks)
 *    (ice_state.F90:141-147), i fastest, ghost cells included, blocks in local-ID order.
 *    Fortran LOGICAL arrays (tmask, umask, iceumask) are passed as int32 0/1.
 *  - all indices are Fortran 1-based.
 *  - return 0 on success, non-zero on error; evpk_last_error() gives the text.  The
 *    library never aborts the process (the Fortran shim maps non-zero to abort_ice,
 *    mpi/ice_exit.F90:22).
 *  - one host thread per context; a context owns its HIP streams and (nranks > 1) its
 *    RCCL communicator.  There is no CPU fallback: without a usable gfx950 device
 *    evpk_create fails.
 */
#ifndef EVPK_H
#define EVPK_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVPK_VERSION 6

/* boundary types: ice_domain.F90 domain_nml ew_boundary_type / ns_boundary_type */
enum { EVPK_BND_CYCLIC = 0, EVPK_BND_OPEN = 1, EVPK_BND_CLOSED = 2, EVPK_BND_TRIPOLE = 3 };

#define EVPK_UNIQUE_ID_BYTES 128

typedef struct evpk_ctx evpk_ctx;

/* Replaces what evp() pulls from ice_blocks / ice_domain / ice_grid:
 *   get_block(blocks_ice(iblk),iblk) -> ilo,ihi,jlo,jhi,i_glob,j_glob  (ice_blocks.F90:22-35, :788)
 *   nblocks, ew/ns boundary types                                       (ice_domain.F90:41-66)
 *   dxt..tinyarea, tarea, uarea, tmask, umask                           (ice_grid.F90:48-77,112-117)
 *   fcor_blk                                                            (ice_dyn_shared.F90:83-84,150)
 * Sharding: ranks own contiguous x-slabs of whole columns (processor_shape slenderX1,
 * ice_distribution.F90:535); rank r's east neighbour is r+1 (cyclic if ew is cyclic). */
typedef struct {
    int32_t nx_global, ny_global;
    int32_t nx_block, ny_block, nblocks;
    int32_t ew_boundary, ns_boundary;
    const int32_t *ilo, *ihi, *jlo, *jhi;      /* [nblocks] */
    const int32_t *iglob_lo, *jglob_lo;        /* [nblocks] this_block%i_glob(ilo), %j_glob(jlo) */
    int32_t rank, nranks;                      /* position in the ring of x-slabs */
    int32_t device;                            /* HIP device ordinal */
    const void *unique_id;                     /* EVPK_UNIQUE_ID_BYTES from evpk_get_unique_id (rank 0), NULL if nranks == 1 */
    const double *dxt, *dyt, *dxhy, *dyhx, *cxp, *cyp, *cxm, *cym;
    const double *tarear, *uarear, *tinyarea, *tarea, *uarea, *fcor;
    const int32_t *tmask, *umask;
    /* optional (NULL allowed): the primary grid lengths HTN, HTE (ice_grid.F90:50-53).  dxt, dyt, dxhy, dyhx, cxp, cyp,
     * cxm, cym are functions of HTN(i,j), HTN(i,j-1), HTE(i,j), HTE(i-1,j) (ice_grid.F90:360-369, :1455, :1533).  If they are
     * given AND reproduce the eight planes above bit for bit on every ocean T cell, the kernels read the two lengths
     * instead of the eight planes (less HBM traffic, identical results); otherwise they are ignored. */
    const double *HTN, *HTE;
} evpk_geom;

/* Replaces the module scalars of ice_dyn_shared.F90:29-81 set by set_evp_parameters
 * (:185-259) and the constants evp reads (ice_constants.F90; a_min, m_min :60-61). */
typedef struct {
    double dt;
    int32_t ndte;
    int32_t revised_evp;
    double revp, ecci, denom1, arlx1i, brlx;
    double cosw, sinw;                         /* AusCOM: namelist variables (ice_dyn_shared.F90:66-72) */
    double rhow, rhoi, rhos, gravit;
    double a_min, m_min;
    int32_t tilt_from_slope;                   /* 1: strtlt = -gravit*umass*ss_tlt (:601-602 / use_ocnslope), 0: geostrophic (:598-599) */
    int32_t wind_on_ugrid;                     /* 1: strairx/y := strax/stray (ice_dyn_evp.F90:226-228), 0: t2ugrid_vector (:240-241) */
    /* ice_strength on the device (used only when evpk_step_in.strength == NULL): the namelist switches of
     * ice_mechred.F90:54-64 (defaults ice_init.F90:273-277: 1, 1, 1, mu_rdg = 3, Cf = 17) and ncat (ice_domain_size) */
    int32_t kstrength, krdg_partic, krdg_redist, ncat;
    double mu_rdg, Cf;
    /* 1: sparse transfers for a host model that keeps the state resident (evpk_upload(in, NULL), page-locked arrays):
     * aice, vice, vsno are uploaded whole, every other input only in the 64x4-cell tiles that hold ice now or held any at
     * the previous call (+ two tiles around), and evpk_download skips tiles that are and were ice-free (they hold the same
     * zeros on both sides).  Identical results provided the T-grid inputs strairxT/yT, aice_init, strength are zero where
     * there is no ice, as CICE leaves them; 0 (default): every cell of every array moves.
     * 2: as 1, and vice, vsno travel in the active tiles too -- only aice is uploaded whole and the tiles are taken from it alone:
     * the host promises vice = vsno = 0 wherever aice = 0 (CICE keeps it so: zap_small_areas, cleanup_itd). */
    int32_t sparse_io;
    int32_t reserved_;
} evpk_params;

/* Per-call inputs: what evp(dt) reads from ice_state / ice_flux / ice_atmo
 * (ice_dyn_evp.F90:70-90).  `strength` is the result of ice_strength (:291-301),
 * physical cells; the library does its halo update (:311).  NULL is allowed for
 * ss_tltx/ss_tlty when tilt_from_slope == 0 and for strax/stray when wind_on_ugrid == 0.
 * strength == NULL: the library evaluates ice_strength itself (ice_mechred.F90:2111-2269) where the reference calls it,
 * from aice, vice and -- for kstrength == 1 -- the thickness distribution aicen, vicen (nx_block, ny_block, ncat,
 * nblocks) and aice0 (ice_state.F90); the host then needs neither evp_prep1 nor the icetmask halo before the call.
 * Its exp() is a fixed < 1 ulp algorithm, so the result can differ from a host intrinsic in the last bit. */
typedef struct {
    const double *aice, *vice, *vsno, *aice_init;
    const double *strairxT, *strairyT, *strax, *stray;
    const double *uocn, *vocn, *ss_tltx, *ss_tlty, *Cdn_ocn;
    const double *strength;
    const double *aicen, *vicen, *aice0;       /* read only when strength == NULL and kstrength == 1 */
} evpk_step_in;

/* In/out prognostic state and outputs: the arrays evp(dt) leaves modified.
 * sigma order: stressp[0..3] = stressp_1..4 etc. (ice_flux.F90:93-97). Any output
 * pointer may be NULL (skipped).  uvel/vvel are written on all cells (ghosts are
 * halo-updated, ice_dyn_evp.F90:392-407); sigma on physical cells and the N/E ghost
 * T-cells the reference computes (ice_dyn_shared.F90:528-537); the rest on physical cells. */
typedef struct {
    double *uvel, *vvel;
    double *stressp[4], *stressm[4], *stress12[4];
    int32_t *iceumask;
    double *divu, *shear, *rdg_conv, *rdg_shear, *prs_sig;
    double *strintx, *strinty, *strocnx, *strocny, *strocnxT, *strocnyT;
    double *strairx, *strairy, *strtltx, *strtlty, *fm;
    double *tmass;                             /* AusCOM: sicemass = tmass (ice_dyn_evp.F90:205-207) */
    double *aiu, *umass, *uvel_init, *vvel_init;
    int32_t *icetmask;
    double *strength;                          /* out, all cells: the strength with its ghost cells halo-updated, as evp leaves it
                                                  (ice_dyn_evp.F90:311-312); may be the array evpk_step_in.strength points to */
} evpk_state;

typedef struct {
    int64_t icellt;          /* active T cells on physical cells of this rank (sum of icellt minus ghost duplicates) */
    int64_t icellu;          /* active U cells of this rank */
    int64_t ncell_slab;      /* physical cells of this rank */
    int32_t nstrips;         /* wave strips launched per subcycle (active) */
    int32_t nstrips_total;
    int32_t subcycles_done;  /* since the last evpk_prep */
    float loop_ms;           /* HIP-event time of the last evpk_subcycle call on the compute stream */
    float kernel_ms;         /* time of the one-subcycle kernel launches (k_subcycle) of that call: HIP events around runs of six
                                consecutive launches (launches 3..8 of every 20 by default; EVPK_TIME_KERNELS=2: every launch, 0: none),
                                span time / launches in the spans x number of launches -- never more than loop_ms */
    int32_t kernel_launches; /* ... and their number */
    float kernel2_ms;        /* the same for the two-subcycle kernels (k_subcycle2p and its tile variants) */
    int32_t kernel2_launches;
    int32_t strip_rows, strip_rows2;   /* strip heights in use: k_subcycle, the two-subcycle kernels (auto-tuned) */
    int32_t nstrips2;
    int32_t zone_cols;                 /* x-slabs: ghost-zone width per side (2 x launches per exchange); 0 = no ghost zones */
    int32_t zone_exchanges;            /* ghost-zone exchanges with the slab neighbours in the last evpk_subcycle call */
    int64_t zone_bytes;                /* bytes this rank sent in them */
    int32_t overlap_split;             /* x-slabs: 1 the exchange launches are split into edge + interior strips on two streams, 0 whole
                                          launches, -1 still trying both (first three evps; EVPK_OVERLAP fixes it) */
    int32_t tile_kernel;               /* 1: the pairs of the last call ran the small-slab tile variant (k_subcycle2t), 0: the marching one */
    int32_t kernel_timed, kernel2_timed;   /* launches of each kind that were actually bracketed by HIP events (kernel_ms / kernel2_ms are
                                          their mean x the number of launches) */
    float bound_ms;                    /* halo / fold / ghost-zone work of the last evpk_subcycle call (pack, transport, unpack): mean of the
                                          HIP-event-timed updates x their number -- what the reference books under timer_bound
                                          (ice_dyn_evp.F90:392-400) */
    int32_t bound_updates;             /* ... and their number */
    int32_t compact_metrics;           /* 1: the kernels rebuild the eight metric planes from HTN / HTE (evpk_geom) */
    int32_t transport;                 /* EVPK_XP_*: what carries the exchanges between ranks */
    int32_t band_row_exchanges;        /* x-slab ranks on a tripole grid: refreshes of the mirror slab in the last evpk_subcycle call -- one message
                                          per rank that owns columns of it, ghost zones included (the mirror rank and its neighbours with equal slabs: up to three ranks), posted
                                          together with the ghost-zone exchange; the fold itself runs inside the pair launches (band_pair) */
    float kernel3_ms;                  /* reserved, always 0 (read by bench.py) */
    int32_t kernel3_launches, kernel3_timed;   /* reserved, always 0 (read by bench.py) */
    int32_t strip_rows3, nstrips3;     /* reserved, always 0 (read by bench.py) */
    int32_t rccl_ranks;                /* ncclCommCount of the context's communicator (0: no RCCL communicator) */
    int32_t device;                    /* hipGetDevice ordinal the context runs on */
    int32_t device_pci;                /* (PCI domain << 16) | (bus << 8) | device of that GPU: distinct per physical device */
    int64_t delivery_checked;          /* EVPK_VERIFY_DELIVERY: values written in place into page-locked caller arrays that were delivered a second
                                          time through the staged path and compared (since evpk_create) ... */
    int64_t delivery_bad;              /* ... and how many of them differed (mode 1: the first one fails the download; mode 2: repaired) */
    int32_t bound_state_rounds;        /* exchange rounds of the last bound_state (evpk_bound_state, evpk_aggregate(bound = 1), evpk_step_dynamics):
                                          0 on one rank; on x-slab ranks 1 while the planes fit one message per partner, one per 14 planes on the
                                          plane-by-plane path */
    int32_t bound_state_planes;        /* planes that bound_state moved: ncat * (3 + ntrcr) */
} evpk_stats;

enum { EVPK_XP_NONE = 0, EVPK_XP_RCCL = 1, EVPK_XP_SHM_RELAY = 2, EVPK_XP_IPC = 3, EVPK_XP_SELF = 4 };

/* rank 0 creates the RCCL id; the host model broadcasts the bytes (MPI_Bcast in CICE,
 * torch.distributed in bench.py) and every rank passes them to evpk_create.
 * Second transport, for ranks that cannot form an RCCL communicator (several ranks on one GPU: tests; or a node whose
 * RCCL bootstrap fails: bench.py's fallback): a unique id that starts with "EVPKSHM:<name>" selects a host-staged relay
 * through the POSIX shared-memory segment /<name> with the same point-to-point / all-gather semantics (correct, slow). */
int evpk_get_unique_id(void *id /* EVPK_UNIQUE_ID_BYTES */);

int evpk_create(const evpk_geom *g, evpk_ctx **out);
/* Two-phase start for nranks > 1: evpk_create with unique_id == NULL allocates and uploads everything but touches no other
 * rank; the host then agrees across ranks (MPI_Allreduce in CICE, gloo in bench.py) that every create succeeded and only
 * then calls evpk_connect, which is collective (communicator / peer mapping, slab starts).  A rank that failed early can
 * therefore not leave the others hanging inside the communicator bootstrap.  evpk_create with a unique_id does both. */
int evpk_connect(evpk_ctx *c, const void *unique_id /* EVPK_UNIQUE_ID_BYTES */);
/* 0 if `device` exists and is a gfx950 part this library can run on (no context needed; error text via evpk_last_error(NULL)) */
int evpk_device_check(int32_t device);
int evpk_set_params(evpk_ctx *c, const evpk_params *p);

/* whole evp(dt): upload + prep + ndte subcycles + finish + download */
int evpk_run(evpk_ctx *c, const evpk_step_in *in, evpk_state *st);

/* the same in stages (bench.py times prep..finish with the data resident in HBM) */
int evpk_upload(evpk_ctx *c, const evpk_step_in *in, const evpk_state *st);  /* st == NULL: inputs only, the state stays resident on the device */
int evpk_prep(evpk_ctx *c);
int evpk_subcycle(evpk_ctx *c, int32_t nsub);   /* advances ksub; the last-subcycle diagnostics fire at ksub == ndte */
int evpk_finish(evpk_ctx *c);
int evpk_download(evpk_ctx *c, evpk_state *st);
int evpk_sync(evpk_ctx *c);

/* On one rank (and on x-slab ranks of a tripole grid) evpk_prep compacts the strip list on the device and returns without
 * waiting for icellt / icellu / nstrips2; evpk_subcycle fills them in when its loop has run.  evpk_get_stats called in between
 * synchronises the compute stream once and returns this evp's counts (never stale ones); it also reports a transport error that
 * an exchange of evpk_prep raised on that path (otherwise reported by evpk_subcycle). */
int evpk_get_stats(evpk_ctx *c, evpk_stats *s);

/* principal_stress (ice_dyn_shared.F90:853-893; called by ice_history for sig1/sig2): normalised principal
 * stresses from the sigma_1 planes and prs_sig resident on the device after evpk_finish / evpk_run.
 * Physical cells of sig1, sig2 (block arrays) are written. */
int evpk_principal_stress(evpk_ctx *c, double *sig1, double *sig2);

/* Row a3 as an entry point of its own: ice_HaloUpdate (mpi/ice_boundary.F90:1331 2DR8, :2451 3DR8) of a block array on the
 * device -- upload, the halo / fold kernels and transports the evp path uses (N-S fill or tripole u-fold, E-W ring between the
 * slab ranks), download.  Collective over the ranks of the context.
 *   a          real(8) (nx_block, ny_block, nblocks) for nz == 0, (nx_block, ny_block, nz, nblocks) for nz >= 1    in / out
 *   field_loc  1 centre, 2 NE corner, 3 N face, 4 E face; field_type 1 scalar, 2 vector, 3 angle (ice_constants.F90:198-220)
 *   fill       the reference's optional fillValue (0 when absent)
 * Written, as by the reference's production (MPI) backend: every ghost cell with a neighbour (its value; `fill` if the
 * neighbour is an eliminated land block), the tripole top row for NE-corner / N-face fields, and the outermost row / column
 * of the block array where nothing else writes (mpi/ice_boundary.F90:1409-1416).  Ghost cells beyond an open / closed
 * boundary that are not on the array's edge (short blocks) and padding cells keep the caller's values.
 * evpk_halo_update_stress: ice_HaloUpdate_stress(array1, array2, halo, field_loc_center, field_type_scalar)
 * (mpi/ice_boundary.F90; ice_dyn_evp.F90:416-481): the tripole north ghost row of a1 from the top row of a2; a ghost cell
 * next to an eliminated land block gets 0; nothing else is touched.
 * Pinned by tests/golden/ref_*.npz (outputs of the reference's own routines). */
/* Both stage through the scratch state planes that evpk_prep primes for the subcycle loop on some paths: call them before
 * evpk_prep or after evpk_finish / evpk_run, never between evpk_prep and the end of the subcycle loop (the reference has no halo
 * update of a foreign field inside evp's loop either, ice_dyn_evp.F90:345-409). */
int evpk_halo_update(evpk_ctx *c, double *a, int32_t nz, int32_t field_loc, int32_t field_type, double fill);
int evpk_halo_update_stress(evpk_ctx *c, double *a1, const double *a2);

/* SURVEY S8 row f-3, first step: transport_upwind (source/ice_transport_driver.F90:634-772) on the velocities the last evp
 * left on the device.  The cell-edge velocities uee, vnn (:688-701) and their halo updates (E face / N face vectors,
 * :703-708) and upwind_field (:1614-1689) run on the GPU; `works` is the work array state_to_work (:1382-1513) fills on the
 * host, real(8) (nx_block, ny_block, narr, nblocks), advected in place on physical cells (ghost cells must be current on
 * entry -- bound_state -- and are left alone; the reference calls bound_state afterwards, :763).  work_to_state /
 * compute_tracers stay with the host's tracer bookkeeping.  Needs HTN and HTE in evpk_geom. */
int evpk_transport_upwind(evpk_ctx *c, double dt, int32_t narr, double *works);

/* transport_upwind WHOLE (ice_transport_driver.F90:634-772): state_to_work (:1382-1513) inside the gather, upwind_field on the
 * device, work_to_state (:1520-1609) with compute_tracers (ice_itd.F90:1359-1501) and bound_state (ice_state.F90:173-238) inside
 * the scatter -- the caller hands over its state arrays as they are:
 *   aice0 (nx_block, ny_block, max_blocks), aicen, vicen, vsnon (nx_block, ny_block, ncat, max_blocks),
 *   trcrn (nx_block, ny_block, ntrcr_dim, ncat, max_blocks) of which tracers 1 .. ntrcr are in use
 *   trcr_depend (ntrcr): 0 area, 1 ice volume, 2 snow volume, 2 + nt: tracer nt (ice_state.F90); nt_Tsfc, nt_alvl, nt_apnd,
 *   nt_fbri: 1-based tracer indices, 0 = not in use; tr_pond_cesm / lvl / topo: the pond scheme flags; Tocnfrz (ice_constants)
 * In / out, every cell of every block: physical cells advected, ghost cells their neighbours' new values (bound_state; aice0 has
 * no halo update in the reference and keeps its ghost cells).  Ghost cells must be current on entry.  Up to 32 tracers. */
int evpk_transport_upwind_state(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                                int32_t nt_Tsfc, int32_t nt_alvl, int32_t nt_apnd, int32_t nt_fbri, int32_t tr_pond_cesm,
                                int32_t tr_pond_lvl, int32_t tr_pond_topo, double Tocnfrz, double *aice0, double *aicen, double *vicen,
                                double *vsnon, double *trcrn);

/* SURVEY S8 row f-3, second step: horizontal_remap (source/ice_transport_remap.F90:309-850), the incremental remapping of
 * transport_remap (ice_transport_driver.F90:258-626), on the velocities the last evp left on the device.
 *
 * evpk_remap_init (once, after evpk_create / evpk_connect): the grid arrays this path reads beyond evpk_geom's -- dxu, dyu
 * (ice_grid.F90) and hm (the land mask as a real, ice_grid.F90) -- block arrays, ghost cells current.
 *
 * evpk_transport_remap replaces the call at ice_transport_driver.F90:513-517 with the same arguments minus uvel, vvel:
 *   mm  real(8) (nx_block, ny_block, 0:ncat, max_blocks): mean mass (aim; category 0 = open water)      in / out
 *   tm  real(8) (nx_block, ny_block, ntrace, ncat, max_blocks): mean tracers (trm); NULL if ntrace = 0   in / out
 *   tracer_type, depend (1-based, 0 = none), has_dependents: (ntrace), as init_transport sets them (:117-187); a tracer
 *   follows the one it depends on
 *   integral_order 1..3, l_dp_midpt: the module parameters of ice_transport_remap.F90:252-262
 *   l_fixed_area: must be 0 (.false., the reference's setting for the B grid, :489-492)
 * Physical cells of mm and tm are advanced in place; ghost cells are read (they are refreshed on the device first, so they
 * need not be current) and left alone -- the reference calls bound_state afterwards (:573).  Up to EVPK_REMAP_MAX_TRACERS
 * tracers.  make_masks, construct_fields, limited_gradient, departure_points, locate_triangles, triangle_coordinates,
 * transport_integrals and update_fields run on the GPU in the Fortran's operation order; state_to_tracers /
 * tracers_to_state and the conservation / monotonicity diagnostics stay with the host's tracer bookkeeping.
 * Returns 0, EVPK_REMAP_BAD_DEPARTURE (a departure point left the neighbouring cells, :1583-1607: the time step is too
 * long; mm, tm untouched), EVPK_REMAP_NEGATIVE_MASS (:3622-3640; mm, tm undefined: the update writes them as it goes) -- the
 * reference aborts the run in both cases -- or 1 with evpk_last_error.  Needs HTN and HTE in evpk_geom. */
#define EVPK_REMAP_MAX_TRACERS 32
#define EVPK_REMAP_BAD_DEPARTURE 11
#define EVPK_REMAP_NEGATIVE_MASS 12
int evpk_remap_init(evpk_ctx *c, const double *dxu, const double *dyu, const double *hm);
int evpk_transport_remap(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrace, double *mm, double *tm, const int32_t *tracer_type,
                         const int32_t *depend, const int32_t *has_dependents, int32_t integral_order, int32_t l_dp_midpt,
                         int32_t l_fixed_area);

/* The same with the state transforms of transport_remap (ice_transport_driver.F90:198-627) on the device too: state_to_tracers
 * (:789-900) inside the gather, tracers_to_state (:908-1003) and bound_state (ice_state.F90:173-238) inside the scatter, so that
 * the caller hands over its state arrays as they are (the optional conservation / monotonicity checks of the reference are
 * compile-time .false., :255-257, and are not reproduced):
 *   aice0 (nx_block, ny_block, max_blocks), aicen, vicen, vsnon (nx_block, ny_block, ncat, max_blocks),
 *   trcrn (nx_block, ny_block, ntrcr_dim, ncat, max_blocks) of which tracers 1 .. ntrcr are in use (ice_state.F90: max_ntrcr / ntrcr)
 *   nt_qsno (1-based), nslyr: the snow enthalpy tracers, advected as trcrn + rhos*Lfresh (:866, :988); rhos_lfresh = that constant
 *   tracer_type, depend, has_dependents: (2 + ntrcr), as init_transport sets them for hice, hsno and the ntrcr tracers
 * In / out, every cell of every block: physical cells whose new area is > 0 are rewritten (the others keep their values, as
 * tracers_to_state leaves them), ghost cells take their neighbours' new values (bound_state).  Ghost cells must be current on
 * entry.  Return values as evpk_transport_remap. */
int evpk_transport_remap_state(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, int32_t nt_qsno, int32_t nslyr,
                               double rhos_lfresh, double *aice0, double *aicen, double *vicen, double *vsnon, double *trcrn,
                               const int32_t *tracer_type, const int32_t *depend, const int32_t *has_dependents,
                               int32_t integral_order, int32_t l_dp_midpt);

/* ridge_ice (source/ice_mechred.F90:101-746), the call of step_ridge (ice_step_mod.F90:1285-1305), on the device:
 * asum_ridging, ridge_prep, ridge_itd, ridge_shift with compute_tracers, ridge_check and the diagnostics, for every block of the
 * context.  cleanup_itd and aggregate, the rest of step_ridge / step_dynamics, follow as evpk_cleanup_itd and evpk_aggregate below.
 *   dt, ndtd                         the dynamics time step and the number of dynamics subcycles (fresh / fhocn average over ndtd * dt)
 *   ncat, ntrcr, ntrcr_dim, trcr_depend, aice0, aicen, vicen, vsnon, trcrn    as for evpk_transport_upwind_state (host arrays, page-locked
 *                                    arrays or device pointers)
 *   t                                the ice_state tracer indices ridge_shift reads, 1-based, 0 = not in use; nslyr snow layers from nt_qsno
 *   hin_max(0:ncat)                  the category boundaries (ice_itd); hin_max(ncat) is taken as 1e8 inside the call, as ridge_prep sets it
 *                                    (:864) -- the caller's array is not written
 *   rdg_conv, rdg_shear              block arrays, or both NULL: the planes the last evp / eap left on the device
 *   diag                             may be NULL, and so may every member; out members are written on listed cells only
 * The cell list is step_ridge's: physical cells with tmask, block by block.  Listed cells are rewritten; ghost cells and unlisted cells
 * keep the caller's values (the reference zeroes trcrn of a whole category slice inside compute_tracers, ice_itd.F90:1401, and calls
 * bound_state afterwards).  krdg_partic, krdg_redist, mu_rdg, rhos come from evpk_params; fsnowrdg, Cs, Gstar, astar, maxraft are the
 * module parameters (:66-83).  Iteration is per block, as ridge_check's flag is per ridge_ice call: while one cell of a block has
 * |asum - 1| >= puny every listed cell of the block ridges again.  compute_tracers runs without nt_Tsfc: a surface temperature is an
 * ordinary area tracer here and is 0, not Tocnfrz, in a category left with aicen <= puny (cleanup_itd's zap_small_areas resets it).
 * exp() is the fixed algorithm of ice_strength on the device.
 * Returns 0; EVPK_RIDGE_STOP with stop[] = {reason, block (1-based), i, j} for the reference's l_stop cases -- 1: aice0 < -puny (:1583),
 * 2: ardg > aicen + puny (:1656), 3: 20 iterations exceeded (:453; i = j = 0), 4: |asum - 1| > puny at the end (:729) -- the failing cell
 * that comes first in (block, j, i) order at the earliest iteration; the state arrays are then undefined (the reference aborts); or 1
 * with evpk_last_error: krdg_redist == 0 (ridge_shift reads hrmax with the index of the compressed list of ridging cells, :1724-1725,
 * :1860-1866, so the reference's result depends on which other cells of the block ridge), aerosol tracers (none can be passed),
 * ntrcr > 32, ncat > 16; nranks > 1 on a context that is not connected yet.
 * x-slab ranks (nranks > 1): ridging never looks beyond a block, so every rank ridges its own blocks and the call is NOT collective; a
 * rank without a block column returns 0 at once; stop[1] is the rank's local block number. */
typedef struct {            /* 1-based tracer indices of ice_state, 0 = not in use */
    int32_t nt_qsno, nslyr, nt_alvl, nt_vlvl, nt_apnd, nt_hpnd, nt_fbri;
    int32_t tr_pond_cesm, tr_pond_lvl, tr_pond_topo;
} evpk_ridge_tracers;
typedef struct {            /* every member may be NULL */
    double *dardg1dt, *dardg2dt, *dvirdgdt, *opening;       /* out, (nx_block,ny_block,nblocks), listed cells only */
    double *fpond, *fresh, *fhocn;                          /* in/out: incremented as :693-720 */
    double *dardg1ndt, *dardg2ndt, *dvirdgndt, *aparticn, *krdgn, *araftn, *vraftn, *aredistn, *vredistn; /* (nx_block,ny_block,ncat,nblocks) */
} evpk_ridge_diag;
#define EVPK_RIDGE_STOP 13
int evpk_ridge_ice(evpk_ctx *c, double dt, int32_t ndtd, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim,
                   const int32_t *trcr_depend, const evpk_ridge_tracers *t, const double *hin_max /* 0:ncat */,
                   const double *rdg_conv, const double *rdg_shear,   /* NULL: the planes the last evp / eap left on the device */
                   double *aice0, double *aicen, double *vicen, double *vsnon, double *trcrn,
                   evpk_ridge_diag *diag, int32_t stop[4] /* out: reason, block, i, j */);

/* The rest of step_ridge / step_dynamics on the device (ice_step_mod.F90:1325-1341, :1152-1189), so that a caller whose state lives in
 * device or page-locked memory runs evp -> transport -> ridge_ice -> cleanup_itd -> bound_state -> aggregate without leaving the GPU.
 * Array conventions as evpk_ridge_ice: host arrays, page-locked arrays or device pointers; staged or used in place.
 *
 * evpk_cleanup_itd: cleanup_itd (source/ice_itd.F90:1514-1769) with limit_aice = .true. for every block of the context: aggregate_area on
 * every cell of the block arrays, the area check (:1646-1670), rebin (:516) with shift_ice (:815) and compute_tracers (:1359),
 * zap_small_areas I and II (:1778) with zap_snow (:2170), zap_snow_temperature (:2274) and the flux increments (:1741-1748).
 *   dt                               what step_ridge passes: dt * ndtd
 *   ncat, ntrcr, ntrcr_dim, trcr_depend, aicen, vicen, vsnon, trcrn    as for evpk_ridge_ice; in / out
 *   t                                the ice_state tracer indices these routines read, 1-based, 0 = not in use; nt_Tsfc is required
 *   hin_max(0:ncat)                  the category boundaries (ice_itd); hin_max(ncat) is not read
 *   k                                constants of ice_constants / ice_therm_shared (drivers/auscom/ice_constants.F90, ice_therm_shared.F90:35);
 *                                    rhoi, rhos come from evpk_params; puny must be 1e-11
 *   tr_aero, nbtrcr, heat_capacity   the reference's arguments of these names; only 0, 0, 1 are accepted
 *   aice0, aice                      (nx_block, ny_block, nblocks), out on every cell
 *   fpond, fresh, fsalt, fhocn       in / out, each may be NULL (not incremented)
 *   first_ice                        int32 (nx_block, ny_block, ncat, nblocks) or NULL: set to 1 where zap_small_areas zaps a category
 * rebin's shiftflag is one flag per block and category boundary: when one cell of a block shifts, shift_ice rewrites the tracers of every
 * cell of the block with aice > puny (as (aicen * trcrn) / aicen) and compute_tracers zeroes those of the others (:1401); the device does
 * the same per block.  Departures: physical ocean cells (tmask) reproduce the reference bit for bit, that zeroing included; land cells
 * and ghost cells of aicen, vicen, vsnon, trcrn keep the caller's values (the reference zeroes their tracers in a block that shifts, and
 * bound_state follows), and the area check and the zaps look at ocean cells only; on a stop the state arrays are undefined (the
 * reference aborts).
 * Returns 0; EVPK_ITD_STOP with stop[] = {reason, block (1-based), i, j} for the reference's l_stop cases: the lowest block that stops,
 * in it the earliest stage in the reference's order (the area check, rebin boundary by boundary -- upward 1 .. ncat-1, then downward --
 * zap_small_areas), and the cell the reference reports: the loop of the area check (:1648-1655) and the error loops of shift_ice
 * (:1040-1126) do not exit and report the LAST failing cell in (j, i) order, zap_small_areas returns at the FIRST in (n, j, i) order.
 * Reasons: 1 aggregate ice area out of bounds (:1650); 2 shift_ice negative daice (:1045), 3 negative dvice (:1066), 4 daice > aicen (:1089),
 * 5 dvice > vicen (:1112); 6 zap: aicen < -puny (:1881); 7 zap: excess area (:2025).  Inputs can reach 1, 3 (a negative vicen under
 * aicen > puny, a donor on the downward pass) and 6.  2, 4, 5 cannot be reached from rebin: it sets daice = aicen > puny and
 * dvice = vicen of the donor, which pass those checks identically; 7 cannot, because aice is checked at :1650 and not recomputed.
 * Or 1 with evpk_last_error: aerosol tracers, nbtrcr > 0, heat_capacity = .false., ntrcr > 32, ncat > 16; nranks > 1 on a context that is
 * not connected yet.  x-slab ranks: as evpk_ridge_ice -- not collective, the rank's own blocks, stop[1] the local block number.
 *
 * evpk_aggregate: the second half of step_dynamics.  bound = 1: bound_state (ice_state.F90:173-238) first -- ice_HaloUpdate, centre
 * scalar, of aicen, trcrn(1:ntrcr), vicen, vsnon (their ghost cells are then in / out; fill 0 next to an eliminated land block) -- then
 * aggregate (ice_itd.F90:246-458) on every cell of every block, ghost cells included: aice, vice, vsno, aice0 (nx_block, ny_block, nblocks)
 * and trcr (nx_block, ny_block, ntrcr_dim, nblocks) are written on every cell, tracers 1 .. ntrcr; the category sums run n outer, the products
 * as written at :356-431.  Then, on physical cells, the tendencies (ice_step_mod.F90:1183-1189): daidtd, dvidtd are in / out -- on entry they
 * hold the pre-dynamics aice, vice -- and so is dagedtd, computed when nt_iage > 0; each may be NULL.
 * x-slab ranks: bound = 1 is COLLECTIVE over the ranks that own block columns (bound_state exchanges, see evpk_bound_state); bound = 0 is
 * not.  A rank without a block column returns 0 at once and joins no exchange.  Refused with 1 and evpk_last_error like the others:
 * nranks > 1 on a context that is not connected yet. */
#define EVPK_HAS_CLEANUP_ITD 1
typedef struct {            /* 1-based tracer indices of ice_state, 0 = not in use; nilyr / nslyr layers from nt_qice / nt_qsno */
    int32_t nt_Tsfc, nt_qice, nilyr, nt_qsno, nslyr, nt_alvl, nt_apnd, nt_hpnd, nt_fbri;
    int32_t tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_brine;
} evpk_itd_tracers;
typedef struct {
    double Tocnfrz, ice_ref_salinity, hs_min, cp_ice, Lfresh, Tmin, puny;
} evpk_itd_constants;
#define EVPK_ITD_STOP 14
int evpk_cleanup_itd(evpk_ctx *c, double dt, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                     const evpk_itd_tracers *t, const double *hin_max /* 0:ncat */, const evpk_itd_constants *k,
                     int32_t tr_aero, int32_t nbtrcr, int32_t heat_capacity,
                     double *aicen, double *vicen, double *vsnon, double *trcrn, double *aice0, double *aice,
                     double *fpond, double *fresh, double *fsalt, double *fhocn, int32_t *first_ice, int32_t stop[4] /* out: reason, block, i, j */);
int evpk_aggregate(evpk_ctx *c, double dt, int32_t bound, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                   const evpk_itd_tracers *t, int32_t nt_iage, double Tocnfrz, double *aicen, double *vicen, double *vsnon, double *trcrn,
                   double *aice, double *vice, double *vsno, double *aice0, double *trcr, double *daidtd, double *dvidtd, double *dagedtd);

/* evpk_linear_itd: the thermodynamic remapping of the thickness distribution, linear_itd (source/ice_therm_itd.F90:69-859 with fit_line
 * :871-958; kitd = 1), as step_therm2 calls it (ice_step_mod.F90:821-871), for every block of the context at once -- the reference calls
 * it block by block and nothing in it looks beyond a block.  A host whose ITD lives on the device runs it there between its vertical
 * thermodynamics and add_new_ice; its output is what evpk_cleanup_itd consumes.  Array conventions as evpk_cleanup_itd.
 *   ncat, ntrcr, ntrcr_dim, trcr_depend, t     as for evpk_cleanup_itd; nt_Tsfc is required when ntrcr > 0
 *   hin_max(0:ncat)                  the category boundaries; hin_max(ncat) is taken as 999.9 inside the call (:208), the array is not written
 *   hi_min                           ice_itd's minimum thickness of category 1
 *   k                                Lfresh, Tocnfrz and puny (must be 1e-11) are read; rhos comes from evpk_params
 *   aicen_init, vicen_init           (nx_block, ny_block, ncat, nblocks), in: the state before the vertical thermodynamics
 *   aicen, vicen, vsnon, trcrn       in / out
 *   aice, aice0                      (nx_block, ny_block, nblocks), out on every cell
 *   fpond                            in / out; read and written only with tr_pond_topo, else it may be NULL
 * What it does: aggregate_area on every cell; the cell list -- physical cells with tmask and aice > puny; for a listed cell hicen_init,
 * hicen, dhicen, the new boundaries hbnew(0:ncat) with the four tests that clear remap_flag, fit_line for category 1 on hicen_init, the
 * category-1 melt da0 (damax clamp, fpond under topo ponds) or the shift of hbnew(0), fit_line for every category, donor / daice / dvice of
 * every boundary with the "very small" resets and the "entire category" rules, in the reference's operation order with p333 = c1 / c3,
 * p666 = c2 / c3; the snow enthalpies of the remap_flag cells carry + rhos * Lfresh through shift_ice; ONE shift_ice call with all
 * ncat - 1 boundaries for every listed cell -- a listed cell whose remap_flag is false still has all its tracers rewritten as
 * (aicen * trcrn) / aicen -- and, in a block with a listed cell, trcrn(1:ntrcr, :) = 0 on the unlisted physical ocean cells
 * (ice_itd.F90:1401); the hi_min clamp of category 1 on remap_flag cells; aggregate_area on every cell.  A block without a listed cell is
 * not touched beyond aice / aice0: its trcrn keeps every bit.
 * Departures: the reference lists every physical cell with aice > puny, this call those with tmask (land carries no ice in CICE;
 * evpk_cleanup_itd draws the same line); land and ghost cells of aicen, vicen, vsnon, trcrn keep the caller's values (the reference
 * zeroes their tracers in a block that calls shift_ice); on a stop the arrays are undefined (the reference aborts).  A boundary that
 * is left with donor = 0 but daice > 0 -- only a negative vicen under aicen > puny can do that, through the second "entire category"
 * rule -- moves nothing (the reference indexes category 0 there).
 * Parity: PINNED to reference-built output.  The call equals, bit for bit on the physical ocean cells, the records of the reference's
 * own compiled linear_itd -- fit_line and the boundary integrals included (tests/golden/ref_litd_*.npz, oracle/ref/Makefile, target therm2;
 * tests/test_therm2_ref_gpu.py), and so does the numpy restatement written from the Fortran (tests/nplitd.py, tests/test_therm2_ref.py).
 * The reference leaves hin_max(ncat) = 999.9 in its module for whatever runs after it (ice_therm_itd.F90:208; recorded with every
 * fixture); this call takes that value inside and leaves the caller's hin_max alone -- no routine after it reads hin_max(ncat).
 * Returns 0; EVPK_LITD_STOP with stop[] = {reason, block (local, 1-based), i, j}: reasons 2 .. 5 are EVPK_ITD_STOP's shift_ice reasons
 * (2 negative daice, 3 negative dvice, 4 daice > aicen, 5 dvice > vicen) -- the lowest block, in it the lowest boundary, in it the first
 * failing check, and the LAST failing listed cell in (j, i) order, as the non-exiting error loops report.  The reference's report loops
 * for reasons 2 and 3 (ice_itd.F90:1046, :1067) read nd as the preceding loop left it, not the cell's own donor; this call uses the
 * cell's own donor.  linear_itd's own rules keep its transfers inside these checks: a daice or dvice below puny times the donor's is
 * reset with donor = 0, one above (1 - puny) times it becomes the whole category, so no input reaches a stop through the remapping
 * of a non-negative state; the checks are made all the same.
 * Or 1 with evpk_last_error, before any copy: a missing pointer, ncat > 16, ntrcr > 32, puny != 1e-11, tr_pond_topo without fpond,
 * ntrcr > 0 without nt_Tsfc; a context of several ranks (nranks > 1) on which evpk_connect has not run.
 * x-slab ranks: not collective -- each rank runs its own blocks, and a rank without a block column returns 0. */
#define EVPK_HAS_LINEAR_ITD 1
#define EVPK_LITD_STOP 15
int evpk_linear_itd(evpk_ctx *c, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim, const int32_t *trcr_depend,
                    const evpk_itd_tracers *t, const double *hin_max /* 0:ncat */, double hi_min,
                    const evpk_itd_constants *k,
                    const double *aicen_init, const double *vicen_init,          /* in, (nx_block,ny_block,ncat,nblocks) */
                    double *aicen, double *vicen, double *vsnon, double *trcrn,  /* in / out */
                    double *aice, double *aice0,                                 /* out, every cell */
                    double *fpond,                                               /* in / out, may be NULL unless tr_pond_topo */
                    int32_t stop[4] /* out: reason, block, i, j */);

/* everything of step_dynamics behind evp / eap (ice_step_mod.F90:1126-1192) in one call, on state staged once.
 *
 * evpk_bound_state: bound_state (ice_state.F90:173-238) alone -- ice_HaloUpdate, centre scalar, fill 0, of aicen, trcrn(1:ntrcr), vicen,
 * vsnon, in ONE launch that works directly between the block arrays (k_bound_state): a ghost cell with a source takes the value of the
 * physical cell it mirrors (through the E-W wrap, or the fold onto row ny_global on a tripole grid; 0 where that cell lies in an
 * eliminated land block), a cell without one takes 0 on the outermost row / column of the array and keeps the caller's value elsewhere;
 * physical cells and the tracer slots ntrcr + 1 .. ntrcr_dim are never written.  Arrays as for evpk_aggregate; trcrn may be NULL when
 * ntrcr == 0.  evpk_aggregate(bound = 1) takes the same path.  EVPK_BOUND_DIRECT=0 (read per call) keeps the plane-by-plane path through
 * the slab, which defines the result.  Returns 1 with evpk_last_error: ncat > 16, ntrcr > 32; nranks > 1 on a context that is not
 * connected yet.
 * x-slab ranks (nranks > 1): COLLECTIVE over the ranks that own block columns; a rank without one returns 0 at once and joins no
 * exchange.  Every rank packs physical cells only -- its westmost and eastmost column for the ring neighbours, on a tripole grid its top
 * row for its fold partners -- into one message per partner; the messages cross once over the context's transport and one launch then
 * fills every ghost cell (k_bound_pack / k_bound_fill).  Planes that do not fit the buffers sized at evpk_connect take further rounds
 * (evpk_stats.bound_state_rounds).  EVPK_BOUND_DIRECT must be the same on every rank: the two paths post different exchanges.  Of the
 * entry points of this section only evpk_bound_state, evpk_aggregate(bound = 1) and evpk_step_dynamics are collective; every collective
 * call ends by checking the transport (a partner that never arrived is an error after 20 s, not a hang).
 *
 * evpk_step_dynamics: [evpk_transport_upwind_state | evpk_transport_remap_state](dt), [evpk_ridge_ice(dt, ndtd)],
 * evpk_cleanup_itd(dt * ndtd), evpk_aggregate(bound = 1, dt), bit for bit, with every caller array the device cannot see copied up at
 * most once and down at most once per call (page-locked and device arrays are used in place).  Every block ridges and then every block
 * cleans up, which equals the reference's per-block step_ridge: neither looks beyond its block.  The members are the arguments of those
 * four entry points under their names there; one struct of borrowed pointers:
 *   advection                        0: none (the state is already transported), 1: transport_upwind, 2: transport_remap
 *   ridge                            0 / 1: ridge_ice
 *   tracer_type .. rhos_lfresh       read when advection == 2
 *   fpond, fresh, fsalt, fhocn, first_ice   in / out, each may be NULL; shared by ridge_ice and cleanup_itd, as the module arrays are
 *   rdg_conv, rdg_shear              both NULL: the planes evp / eap left on the device
 *   diag                             may be NULL; its fpond / fresh / fhocn members are ignored in favour of the ones above
 * A stop of a stage returns that stage's code (EVPK_REMAP_BAD_DEPARTURE, EVPK_REMAP_NEGATIVE_MASS, EVPK_RIDGE_STOP, EVPK_ITD_STOP) with
 * stop[0] = the stage (1 transport, 2 ridge, 3 cleanup) and stop[1..4] that stage's four numbers (0 for transport); later stages do not
 * run and the arrays are undefined.  A refused call (return 1 with evpk_last_error: nranks > 1 on a context that is not connected
 * yet, advection / ridge out of range, a missing pointer, anything one of the stages refuses) is refused before the first copy and
 * touches nothing.
 * x-slab ranks: COLLECTIVE -- every rank that owns block columns calls it with the same advection / ridge / ncat / ntrcr; a rank without
 * a block column returns 0 at once.  Stops are per rank, as the reference's l_stop is per task: a rank whose transport, ridging or
 * cleanup stage stops skips the computation that is left but still posts every remaining exchange of the call (aggregate's
 * bound_state) with whatever its arrays hold, then returns its stage's code and stop[] (stop[2] its local block number).  The other
 * ranks return 0; their ghost cells next to the stopped rank are undefined.  The host aborts the run on any non-zero return, as the
 * reference does (abort_ice). */
#define EVPK_HAS_STEP_DYNAMICS 1
#define EVPK_HAS_STEP_DYNAMICS_RANKS 1
int evpk_bound_state(evpk_ctx *c, int32_t ncat, int32_t ntrcr, int32_t ntrcr_dim,
                     double *aicen, double *vicen, double *vsnon, double *trcrn);
typedef struct {
    int32_t advection;
    int32_t ridge;
    double dt; int32_t ndtd;
    int32_t ncat, ntrcr, ntrcr_dim; const int32_t *trcr_depend;
    evpk_itd_tracers t; int32_t nt_vlvl, nt_iage;
    const double *hin_max; evpk_itd_constants k;
    int32_t tr_aero, nbtrcr, heat_capacity;                   /* as for evpk_cleanup_itd: only 0, 0, 1 are accepted */
    const int32_t *tracer_type, *depend, *has_dependents; int32_t integral_order, l_dp_midpt; double rhos_lfresh;
    double *aice0, *aicen, *vicen, *vsnon, *trcrn;            /* in / out */
    double *aice, *vice, *vsno, *trcr;                        /* out */
    double *daidtd, *dvidtd, *dagedtd;                        /* in / out, may be NULL */
    double *fpond, *fresh, *fsalt, *fhocn; int32_t *first_ice;
    const double *rdg_conv, *rdg_shear;
    evpk_ridge_diag *diag;
} evpk_dyn_args;
int evpk_step_dynamics(evpk_ctx *c, const evpk_dyn_args *a, int32_t stop[5] /* out: stage, reason, block, i, j */);

/* step_therm2 (source/ice_step_mod.F90:741-995) in one call, on state staged once.
 *
 * evpk_new_ice_lateral_melt: what step_therm2 does between linear_itd and cleanup_itd, in ONE launch, for every block of the context:
 * add_new_ice (source/ice_therm_itd.F90:1239-1850, l_conservation_check = .false.), lateral_melt (:1043-1217) and, when ncat == 1,
 * reduce_area (ice_itd.F90:743-806).  It runs on the aice / aice0 it is given (aggregate_area is the caller's, or evpk_linear_itd's),
 * has no stop and is not collective; it is there for a host that keeps its own linear_itd.  Array conventions as evpk_cleanup_itd.
 * Per physical ocean cell (tmask), in the reference's order and operation order:
 *   add_new_ice   hi0max = 0.9 hin_max(1) (bignum = 1e30 for ncat == 1); qi0new = -rhoi * Lfresh and Sprofile = salinz(1:nilyr) for
 *                 ktherm == 1; for ktherm == 2 Si0new from sss (both cases of :1468-1472), Ti = min(liquidus_temperature_mush(Si0new /
 *                 phi_init), -0.1), qi0new = enthalpy_mush(Ti, Si0new) through liquid_fraction and liquidus_brine_salinity_mush
 *                 (ice_therm_mushy.F90:3687-3756, :3903-3918) with that module's liquidus parameters compiled in (:43-123, derived in its
 *                 expression order; the merge masks are multiplications); fnew, vi0new, frazil; frz_onset when given; the update_ocn_f /
 *                 mushy-return increments of fresh, fsalt; the distribution decision with its four outcomes; the surplus loop over all
 *                 categories (iage, vlvl, the volume, then update_vertical_tracers on qice and sice for ktherm == 2 or the bulk mix for
 *                 ktherm == 1); the category-1 merge (Tsfc and FY with their clamps, iage, alvl / vlvl, the three pond rules, qice / sice)
 *   lateral_melt  for n = 1 .. ncat, where rside > 0: dfresh, dfsalt, dfpond under topo ponds, meltl, the three state scalings, then
 *                 fhocn over the ice layers and the snow layers with the scaled vicen / vsnon; n outer, the layers inner
 *   reduce_area   when ncat == 1, with aicen_init / vicen_init
 * A cell with frzmlt <= 0 and rside <= 0 writes frazil (0) and nothing else and reads no tracer.  nt_iage, nt_FY, nt_vlvl (with
 * t.nt_alvl) switch tr_iage, tr_FY, tr_lvl; ntrcr == 0 leaves every tracer statement out.
 * Departures: (a) lateral_melt's cell list is physical cells with tmask and rside > 0 (the reference: every physical cell with
 * rside > 0; land carries no ice); land and ghost cells of every array keep the caller's values.  (b) In the ktherm /= 2 surplus loop the
 * reference indexes qi0new and Sprofile with the counter of the compressed surplus list, not with the cell's own index (:1688, :1691):
 * harmless for qi0new, one constant there, but Sprofile then is the salinz profile of another ocean cell of the block.  This call uses the
 * cell's own profile; the two agree whenever salinz is horizontally uniform, which is how init_thermo_vertical fills it
 * (ice_therm_vertical.F90:575-591) -- salinz must be horizontally uniform for parity.  (c) add_new_ice_bgc, aerosols and bgc tracers
 * are refused.
 * Parity: PINNED to reference-built output.  add_new_ice, lateral_melt, reduce_area and the mushy liquidus equal, bit for bit on the
 * physical ocean cells, the records of the reference's own compiled routines (tests/golden/ref_therm2_*.npz, oracle/ref/Makefile, target therm2),
 * each on its own and chained, and evpk_step_therm2 equals the record after cleanup_itd (tests/test_therm2_ref_gpu.py); the numpy
 * restatement written from the Fortran (tests/nptherm2.py) equals the records stage by stage (tests/test_therm2_ref.py).  The liquidus
 * parameters derived in the module's expression order are the values the Fortran compiler folds: no difference was found.  The
 * reference's AusCOM build fixes cp_ocn = 3989.24495292815 (drivers/auscom/ice_constants.F90:30); the records are made with it, and a
 * caller that wants that build's numbers passes it.  Unpinned stay: step_therm2's call order (the driver restates it), a horizontally
 * non-uniform salinz (departure (b)), aerosols / bgc (refused), l_conservation_check = .true. (compile-time .false. in the reference).
 *
 * evpk_step_therm2: the frain line (ice_step_mod.F90:804-809: fresh += frain * aice on every cell, ghost cells included, on the aice of
 * entry), aggregate_area on every cell, evpk_linear_itd when kitd == 1, evpk_new_ice_lateral_melt, evpk_cleanup_itd(dt) -- bit for bit
 * those entry points called in that order, with every caller array the device cannot see copied up at most once and down at most once
 * (page-locked and device arrays are used in place).  fresh is the reference's sum in its order: frain, add_new_ice, lateral_melt
 * n = 1 .. ncat, cleanup_itd.  A stop returns the stage's code, EVPK_LITD_STOP or EVPK_ITD_STOP, with stop[0] = 1 (linear_itd) or 3
 * (cleanup_itd) and stop[1..4] that stage's numbers; later stages do not run and the arrays are undefined.
 * Members (one struct of borrowed pointers; arrays (nx_block, ny_block[, ncat | nilyr+1], nblocks)):
 *   kitd (0 / 1), ktherm (1 / 2), update_ocn_f; dt, yday, hi_min, hfrazilmin, phi_init, dSin0_frazil, cp_ocn
 *   ncat, ntrcr, ntrcr_dim, trcr_depend, t, nt_sice, nt_iage, nt_FY, nt_vlvl; hin_max(0:ncat); k (puny must be 1e-11)
 *   tr_aero, nbtrcr, heat_capacity, skl_bgc      only 0, 0, 1, 0 are accepted; rhow, rhoi, rhos come from evpk_params
 *   aicen_init, vicen_init                       in (read by linear_itd and reduce_area)
 *   aicen, vicen, vsnon, trcrn, aice, aice0      in / out
 *   frain, frzmlt, Tf, sss, rside, salinz        in; salinz (nx_block, ny_block, nilyr+1, nblocks)
 *   frazil, frz_onset, meltl, fpond, fresh, fsalt, fhocn, first_ice     in / out
 * May be NULL (that increment is skipped): frain; frz_onset (with it yday is not read); fpond unless tr_pond_topo; first_ice.
 * Both return 1 with evpk_last_error before any copy, touching nothing: tr_brine or skl_bgc, tr_aero, nbtrcr > 0, heat_capacity = 0,
 * ktherm not 1 or 2, a missing pointer, nt_Tsfc / nt_qice / nt_sice not given while ntrcr > 0, nilyr or nslyr > 8, ncat > 16,
 * ntrcr > 32, puny != 1e-11, a context of several ranks (nranks > 1) on which evpk_connect has not run.
 * x-slab ranks: neither call is collective -- each rank runs its own blocks, and a rank without a block column returns 0. */
#define EVPK_HAS_STEP_THERM2 1
typedef struct {
    int32_t kitd, ktherm, update_ocn_f;
    double dt, yday, hi_min, hfrazilmin, phi_init, dSin0_frazil, cp_ocn;
    int32_t ncat, ntrcr, ntrcr_dim; const int32_t *trcr_depend;
    evpk_itd_tracers t; int32_t nt_sice, nt_iage, nt_FY, nt_vlvl;
    const double *hin_max; evpk_itd_constants k;
    int32_t tr_aero, nbtrcr, heat_capacity, skl_bgc;
    const double *aicen_init, *vicen_init;                    /* in */
    double *aicen, *vicen, *vsnon, *trcrn, *aice, *aice0;     /* in / out */
    const double *frain, *frzmlt, *Tf, *sss, *rside, *salinz; /* in; frain may be NULL */
    double *frazil, *frz_onset, *meltl, *fpond, *fresh, *fsalt, *fhocn; int32_t *first_ice;
} evpk_therm2_args;
int evpk_new_ice_lateral_melt(evpk_ctx *c, const evpk_therm2_args *a);
int evpk_step_therm2(evpk_ctx *c, const evpk_therm2_args *a, int32_t stop[5] /* out: stage, reason, block, i, j */);

/* thermo_vertical (source/ice_therm_vertical.F90:79-531) as step_therm1 calls it once per category and block
 * (source/ice_step_mod.F90:364-540), in ONE launch for every category of every block of the context, on state staged once: the BL99
 * path -- ktherm = 1, heat_capacity = .true., calc_Tsfc = .true., l_brine = .true.  With it a host whose thickness distribution lives
 * in device memory runs the vertical thermodynamics, evpk_step_therm2 and evpk_step_dynamics with no state transfer.
 * Per listed cell and category n = 1 .. ncat, in the reference's order and operation order (k_thermo_vertical, csrc/evpk_therm1.hip):
 *   init_vertical_profile (:845-1273)       hin, hsn, hilyr, hslyr; zqsn / zTsn with the hs_min rule and the zTsn > 0 reset; zSin, Tmlts,
 *                                           zqin; zTin through calculate_Tin_from_qin (ice_therm_shared.F90:62-90) with the zTin > 0 reset;
 *                                           einit; the five stop checks
 *   temperature_changes (ice_therm_bl99.F90:51-928)   conductivity (:940-1062; conduct 0 'MU71', 1 'bubbly'); the move of excess Iswabs /
 *                                           Sswabs into fswsfc with the non-CCSM constants frac = 0.9, dTemp = 0.02; the iteration up to
 *                                           nitermax = 500: surface_heat_flux and dsurface_heat_flux_dTsf (ice_therm_shared.F90:98-226),
 *                                           the Tsf = -puny reset, get_matrix_elements_calc_Tsfc (:1172-1480, all four l_snow x l_cold
 *                                           cases), tridiag_solver (:1763-1840), conditions 1 - 5 with avg_Tsf / avg_Tsi, dqmat / einex,
 *                                           reduce_kh and the reduced conductivity of the next iteration -- a cell leaves the iteration
 *                                           when its `converged` is true; the final update of flwoutn, fsensn, flatn
 *   thickness_changes (:1283-2020)          condensation onto snow or ice, bottom growth with qbot and qbotmax, congel, frz_onset,
 *                                           sublimation and top melt of snow then ice, bottom melt of ice then snow, mlt_onset, melts,
 *                                           meltt, meltb, fhocnn, snowfall, dsnow, freeboard (:2031-2170, snoice), both adjust_enthalpy
 *                                           calls (:2177-2280), efinal.  einter is not built: it is only printed
 *   conservation_check_vthermo (:2283-2406) live code in the reference, hence a stop here
 *   :482-503                                freshn, fsaltn, fhocnn, and fpond under tr_pond_topo (a category that melted away)
 *   update_state_vthermo (:2417-2540)       given Tbot as its Tf: a category that melts away gets zero state and Tsfc = Tbot
 * iage passes through unchanged (the reference's update is commented out, :1599, :2154).  sss is not read when ktherm = 1.
 * Operation order: min / max are a comparison and a select; exp is the fixed algorithm of ice_strength (dev_exp); x**2, x**3 and x**4
 * are x*x, x*x*x and (x*x)*(x*x); sqrt is the IEEE one.
 * Departure: the cell list of ice_step_mod.F90:378-389 (physical cells with aicen(i,j,n) > puny) also requires tmask, as in
 * evpk_new_ice_lateral_melt; land and ghost cells of the in / out arrays keep the caller's values.
 * The reference zeroes flwoutn, evapn, freshn, fsaltn, fhocnn, fsensn, flatn, fsurfn, fcondtopn, melttn, meltsn, meltbn, congeln,
 * snoicen, dsnown on every cell of the block before it starts (:251-280, ice_step_mod.F90:366-371).  Here they are per-category planes
 * (nx_block, ny_block, ncat, nblocks), written on every cell, ghost cells included: zero wherever the cell is not listed.
 * Constants: rhow, rhoi, rhos come from evpk_params; ice_ref_salinity, hs_min, cp_ice, Lfresh, Tmin, puny from k.  Compiled in
 * (drivers/cice/ice_constants.F90 unless another file is named): cp_ocn = 4218 (:29), Lvap = 2.501e6 (:52), Tffresh = 273.15 (:50),
 * TTTice = 5897.8 (:92), qqqice = 11637800 (:91), emissivity = 0.95 (:27), stefan_boltzmann = 567e-10 (:49), depressT = 0.054 (:31),
 * ksno = 0.30 (:75), kice = 2.03 (:71); betak = 0.13, kimin = 0.10 (source/ice_therm_bl99.F90:27-28), Tsf_errmax = 5e-4 (:152),
 * nitermax = 500 (:148); ferrmax = 1e-3 (source/ice_therm_shared.F90:31).
 * **Parity is unpinned for all of thermo_vertical**: it is held bit for bit to a numpy restatement written from the Fortran
 * (tests/nptherm1.py); no reference-built record of it exists yet.
 * Members (one struct of borrowed pointers; arrays (nx_block, ny_block[, ncat], nblocks) unless given):
 *   dt, yday, ktherm, calc_Tsfc, heat_capacity, l_brine (only 1, 1, 1, 1 are accepted), conduct (0 MU71 / 1 bubbly), min_salin
 *   ncat, ntrcr, ntrcr_dim, t (nt_Tsfc, nt_qice, nilyr, nt_qsno, nslyr; nt_apnd, nt_hpnd with tr_pond_topo), nt_sice, k
 *   aicen, vicen, vsnon, trcrn                               in / out
 *   flw, potT, Qa, rhoa, fsnow, fbot, Tbot, sss              in, 2-D
 *   shcoef, lhcoef                                           in, per category
 *   fswsfcn, fswintn, Sswabsn (nx_block, ny_block, nslyr, ncat, nblocks), Iswabsn (.., nilyr, ncat, ..)     in / out, per category
 *   fpond (may be NULL unless tr_pond_topo), mlt_onset, frz_onset     in / out, 2-D
 *   the fifteen per-category outputs named above             out
 * Returns 0; or EVPK_THERMO_STOP with stop[] = {reason, block (local, 1-based), category, i, j}: reason 1 zTsn > Tmax, 2 zTsn < Tmin,
 * 3 zSin < min_salin - puny, 4 zTin > Tmlts, 5 zTin < Tmin, 6 no convergence after nitermax, 7 ferr > ferrmax -- the stop the reference
 * would meet first: the lowest block, in it the lowest category, in it the reference's check sequence (reason 1 over the snow layers,
 * reason 2 over the snow layers, then ice layer by ice layer reasons 3, 4, 5, then 6, then 7), in it the first cell with j outer and i
 * inner.  After a stop the arrays are undefined.  (Reason 4 cannot occur: zTin = min(root, Tmlts) never exceeds Tmlts.  The check is made.)
 * Or 1 with evpk_last_error, before any copy, touching nothing: ktherm != 1; calc_Tsfc, heat_capacity or l_brine not 1; conduct not 0
 * or 1; a missing pointer; nt_Tsfc, nt_qice, nt_qsno or nt_sice not given; nilyr or nslyr > 8; ncat > 16; ntrcr > 32; puny != 1e-11;
 * tr_pond_topo without fpond, nt_apnd, nt_hpnd; a context of several ranks (nranks > 1) on which evpk_connect has not run.
 * x-slab ranks: not collective -- each rank runs its own blocks, and a rank without a block column returns 0.
 * Out of scope: frzmlt_bottom_lateral (its deltaT**m2 is a real power: it needs a fixed-algorithm pow first); atmo_boundary_layer,
 * increment_age, update_FYarea, the pond routines, merge_fluxes (with these step_therm1 becomes one call: evpk_step_therm1, row f-11 below); ktherm = 2, zero-layer
 * thermodynamics, calc_Tsfc = .false., fresh ice (l_brine = .false.); aerosols. */
#define EVPK_HAS_THERMO_VERTICAL 1
#define EVPK_THERMO_STOP 16
typedef struct {
    double dt, yday;
    int32_t ktherm, calc_Tsfc, heat_capacity, l_brine, conduct;
    double min_salin;
    int32_t ncat, ntrcr, ntrcr_dim;
    evpk_itd_tracers t; int32_t nt_sice;
    evpk_itd_constants k;
    double *aicen, *vicen, *vsnon, *trcrn;                                    /* in / out */
    const double *flw, *potT, *Qa, *rhoa, *fsnow, *fbot, *Tbot, *sss;         /* in */
    const double *shcoef, *lhcoef;                                            /* in, per category */
    double *fswsfcn, *fswintn, *Sswabsn, *Iswabsn;                            /* in / out, per category */
    double *fpond, *mlt_onset, *frz_onset;                                    /* in / out */
    double *flwoutn, *evapn, *freshn, *fsaltn, *fhocnn, *fsensn, *flatn, *fsurfn, *fcondtopn;     /* out, per category, every cell */
    double *melttn, *meltsn, *meltbn, *congeln, *snoicen, *dsnown;
} evpk_thermo_args;
int evpk_thermo_vertical(evpk_ctx *c, const evpk_thermo_args *a, int32_t stop[5] /* out: reason, block, category, i, j */);

/* step_therm1 (source/ice_step_mod.F90:154-733) in ONE call, three launches on state staged once: k_therm1_open,
 * k_thermo_vertical (row f-10, unchanged), k_therm1_merge (csrc/evpk_therm1s.hip).  With it a host whose thickness distribution lives in
 * device memory calls evpk_step_therm1, evpk_step_therm2 and evpk_step_dynamics and moves only 2-D forcing and 2-D fluxes.
 *   k_therm1_open   aice_init, aicen_init, vicen_init (:272-285: copies on every cell of the block arrays, ghost cells included);
 *                   frzmlt_bottom_lateral (source/ice_therm_vertical.F90:611-834), AusCOM branch cpchr = -cp_ocn rhow chio: rside = 0,
 *                   Tbot = Tf, fbot = 0 on every cell, then on physical cells with aice > puny and frzmlt < 0 deltaT, ustar with ustar_min,
 *                   fbot clamped by frzmlt, wlat = m1 deltaT**m2 (the real power: evpk_pow_pos), rside clamped to [0, 1], etot and fside
 *                   over the categories in order (snow layers before ice layers), the xtmp limiting;
 *                   per category on the cell list of :378-389 AND tmask (the stated departure of evpk_thermo_vertical, kept so that
 *                   all kernels list the same cells): atmo_boundary_layer (source/ice_atmo.F90:82-483; sfctype 'ice', highfreq and
 *                   formdrag .false.) -- vmag = max(1, wind), rdn = vonkar / log(zref / iceruf) computed as written, Cdn_atm = rdn rdn,
 *                   natmiter iterations of hol with its sign / min(abs, 10) clamp, stable, xqq, psimhs, psimhu, psixhu, rd, rh, re; with
 *                   calc_strair strairxn, strairyn, Cdn_atm_ratio_n, without it (AusCOM, :458-464) strairxn = strairyn = 0; shcoef,
 *                   lhcoef, Trefn, Qrefn, Urefn; then increment_age (tr_iage) and update_FYarea (tr_FY; yday, dt / secday, lmask_n,
 *                   lmask_s).  atmo_boundary_layer of category n reads only Tsfc(n) of entry and frzmlt_bottom_lateral only the state
 *                   of entry: running all of this before the first thermo_vertical is the reference's result, not a reordering.
 *   k_therm1_merge  per category in order: fswabsn = fswsfcn + fswintn + fswthrun (:565-571; fswsfcn and fswintn as k_thermo_vertical
 *                   left them); compute_ponds_cesm under tr_pond_cesm (source/ice_meltpond_cesm.F90:61-197) on its own list -- aicen >
 *                   puny on the state AFTER the vertical thermodynamics, with tmask -- rfrac from rfracmin, rfracmax; merge_fluxes
 *                   (source/ice_flux.F90:681-831): all 22 accumulations, weighted with aicen_init, over the list of entry; flwout with
 *                   its (1 - emissivity) flw term.  One thread per cell, categories in order: the sums carry the reference's bits.
 * The eight per-category results of atmo_boundary_layer (shcoef, lhcoef, strairxn, strairyn, Cdn_atm_ratio_n, Trefn, Qrefn, Urefn) are
 * locals of step_therm1.  Here they are per-category planes the library owns (one pool, grown once), or the caller's where given; they
 * are ZERO wherever the cell is not listed.  The Fortran's block-wide `icells > 0` test (:391) only decides whether locals that nobody
 * reads hold zeros or the previous category's values.  Cdn_atm_ratio_n without calc_strair is left unset by the reference; here it is 0.
 * Operation order: the Fortran's; min / max are a comparison and a select; sign(a, b) is copysign-exact, b = -0 included; x**2 is x*x; exp
 * is dev_exp; log, atan and the real power are the fixed algorithms of csrc/evpk_fmath2.h (within 1 ulp of glibc on the CPU, held to 2);
 * sqrt is the IEEE one.
 * Constants: rhow, rhoi, rhos from evpk_params; puny from tv.k.  Compiled in (drivers/cice/ice_constants.F90 unless another file is named):
 * vonkar = 0.4 (:47), zref = 10 (:76), iceruf = 0.0005 (:64), zvir = 0.606 (:46), cp_air = 1005 (:25), cp_wv = 1810 (:48), gravit = 9.80616
 * (:36), Lsub = 2.835e6 (:51), pi (:153), secday = 86400 (:41), rhofresh = 1000 (:45), Timelt = 0 (:54), cp_ocn, Tffresh, qqqice, TTTice and
 * emissivity as row f-10; m1 = 1.6e-6, m2 = 1.36, floediam = 300, floeshape = 0.66 (source/ice_therm_vertical.F90:682-687); zTrf = 2
 * (source/ice_atmo.F90:196); Td = 2, rexp = 0.01, dpthhi = 0.9 (source/ice_meltpond_cesm.F90:116-119).
 * The frain / fsnow scaling of :294-314 is behind ACCESS, which this project's build of the reference does not define: it is left out.
 * **Parity unpinned**: no recipe under oracle/ builds these routines; the call is held bit for bit to a numpy restatement written from
 * the Fortran (tests/nptherm1s.py, which calls tests/nptherm1.py for thermo_vertical).
 * Members: tv -- evpk_thermo_args, whose shcoef, lhcoef, fbot, Tbot may be NULL; where given they RECEIVE what k_therm1_open computed
 *   (they are outputs here, despite the const of the member);
 *   aice, frzmlt, sst, Tf, strocnxT, strocnyT, uatm, vatm, wind, zlvl, frain   in, 2-D (frain only with tr_pond_cesm; else may be NULL)
 *   fswthrun                                                  in, per category
 *   lmask_n, lmask_s                                          in, int32 block arrays as evpk_geom's tmask (only with tr_FY; else may be NULL)
 *   Cdn_atm                                                   in / out, 2-D: written on listed cells
 *   rside, aice_init (2-D), aicen_init, vicen_init (per category)     out, every cell
 *   strairxT .. snoice: merge_fluxes' 22 cumulative planes    in / out, 2-D, physical ocean cells
 *   strairxn, strairyn, Cdn_atm_ratio_n, Trefn, Qrefn, Urefn  out if not NULL, per category, every cell
 *   chio, ustar_min, hi_min, pndaspect, rfracmin, rfracmax; natmiter (the reference's default: 5), calc_strair, tr_iage, tr_FY, nt_iage,
 *   nt_FY; tr_pond_cesm is tv.t.tr_pond_cesm; the flags of what is refused: formdrag, highfreq, atmbndy_constant, fbot_xfer_Cdn_ocn, tr_aero
 * Returns 0; or EVPK_THERMO_STOP with the stop[] of evpk_thermo_vertical unchanged -- only k_thermo_vertical can stop; k_therm1_merge is
 * not launched after a stop, and the arrays are undefined.
 * Or 1 with evpk_last_error, before any copy, touching nothing: everything evpk_thermo_vertical refuses; formdrag; highfreq; atmbndy =
 * 'constant'; fbot_xfer_type = 'Cdn_ocn'; tr_pond_lvl; tr_pond_topo (its compute_ponds_topo is a row of its own); aerosols; natmiter < 1;
 * a tracer flag without its index (tr_iage / nt_iage, tr_FY / nt_FY, tr_pond_cesm / nt_apnd, nt_hpnd); a missing pointer.
 * x-slab ranks: not collective -- a rank without a block column returns 0.
 * Out of scope: neutral_drag_coeffs (formdrag), highfreq coupling, atmo_boundary_const, compute_ponds_lvl, compute_ponds_topo and the
 * topo collection lines of :644-669, update_aerosol, set_sfcflux (calc_Tsfc = .false.), prep_radiation and the shortwave routines,
 * ktherm = 2. */
#define EVPK_HAS_STEP_THERM1 1
typedef struct {
    evpk_thermo_args tv;
    const double *aice, *frzmlt, *sst, *Tf, *strocnxT, *strocnyT, *uatm, *vatm, *wind, *zlvl, *frain;       /* in */
    const double *fswthrun;                                                   /* in, per category */
    const int32_t *lmask_n, *lmask_s;                                         /* in */
    double *Cdn_atm;                                                          /* in / out */
    double *rside, *aice_init, *aicen_init, *vicen_init;                      /* out */
    double *strairxT, *strairyT, *Cdn_atm_ratio, *fsurf, *fcondtop, *fsens, *flat, *fswabs, *flwout, *evap, *Tref, *Qref, *Uref;      /* in / out */
    double *fresh, *fsalt, *fhocn, *fswthru, *meltt, *meltb, *melts, *congel, *snoice;
    double *strairxn, *strairyn, *Cdn_atm_ratio_n, *Trefn, *Qrefn, *Urefn;    /* out if not NULL, per category */
    double chio, ustar_min, hi_min, pndaspect, rfracmin, rfracmax;
    int32_t natmiter, calc_strair, tr_iage, tr_FY, nt_iage, nt_FY;
    int32_t formdrag, highfreq, atmbndy_constant, fbot_xfer_Cdn_ocn, tr_aero;
} evpk_therm1_args;
int evpk_step_therm1(evpk_ctx *c, const evpk_therm1_args *a, int32_t stop[5] /* out: reason, block, category, i, j */);

/* the shortwave of ice_step (kernels in csrc/evpk_rad.hip, host layer in csrc/evpk_api_column.hip).
 * With it the per-category radiation arrays that
 * evpk_step_therm1 reads (fswsfcn, fswintn, fswthrun, Sswabsn, Iswabsn) are made on the device from the state the project leaves there.
 *
 * evpk_step_radiation: step_radiation (source/ice_step_mod.F90:1364-1524) on its calc_Tsfc / not-dEdd branch -- shortwave_ccsm3
 * (source/ice_shortwave.F90:425-646; shortwave = 'default', reference/input_templates/gx1/ice_in.v4.1:116-119) -- and the albedo lines
 * of coupling_prep that follow it at once in the reference's ice_step (drivers/auscom/CICE_RunMod.F90:503-548, :564-567, :582-586), in
 * ONE launch (k_shortwave_ccsm3) for every category of every block: one thread per cell that walks the categories in order.
 *   initialisation     on EVERY cell of the block arrays, ghost cells included (ice_step_mod.F90:1408-1423, ice_shortwave.F90:523,
 *                      :538, :737-777, :1106-1116): coszen = 0.5; alvdrn, alidrn, alvdfn, alidfn = the ocean albedo of the cell;
 *                      albicen, albsnon, fswsfcn, fswintn, fswthrun, every layer of Sswabsn, Iswabsn and fswpenln = 0
 *   ocean albedo       the AusCOM build reads the 2-D ocn_albedo2D (:759-772, :798, :814), the stock build the scalar albocn: where
 *                      ocn_albedo2D is NULL, albocn is used on every cell
 *   cell list          per category (:527-536): physical cells with aicen > puny AND tmask -- the stated departure of
 *                      evpk_thermo_vertical, kept so that every column kernel lists the same cells
 *   compute_albedos    (:786-859) hi, hs; fh = min(atan(4 hi) / fhtan, 1), fhtan = atan(4 ahmax), both through evpk_atan; albo; the
 *                      bare-ice albedos; fT = min(dTs / dT_melt - 1, 0); the max against the ocean albedo; the snow albedos under
 *                      hs > puny; direct = diffuse; asnow = hs / (hs + snowpatch); the four combined albedos; albicen, albsnon with
 *                      the four awt* weights summed left to right
 *   constant_albedos   (:964-1009) with albedo_constant (albedo_type = 'constant') instead
 *   absorbed_solar     (:1118-1211) asnow again; swabsv, swabsi, swabs with the parentheses as written; fswpenvdr, fswpenvdf
 *                      multiplied left to right; fswpen, fswsfc; per layer k hilyr = hi / nilyr, tranbot = exp(((-kappav) hilyr) k)
 *                      through dev_exp, Iswabs(k) = fswpen (trantop - tranbot), fswpenl(k), fswpenl(k+1); fswthru = fswpen tranbot,
 *                      fswint = fswpen - fswthru.  Sswabsn stays zero: the CCSM3 scheme absorbs nothing in snow layers
 *   aggregation        every cell, categories in order: alvdf, alidf, alvdr, alidr += al*n aicen; albice, albsno likewise under
 *                      coszen > puny (always true here; the test is kept); scale_factor = swvdr (1 - alvdr) + swvdf (1 - alvdf) +
 *                      swidr (1 - alidr) + swidf (1 - alidf) in that order.  alvdr_ai .. alidf_ai are plain copies of the four sums
 *                      (:564-567): they are not separate outputs, the caller aliases them
 * Operation order: the Fortran's; min / max are a comparison and a select; x**2 does not occur.
 * Compiled in: kappav = 1.4, Timelt = 0 (drivers/auscom/ice_constants.F90:82, :65); dT_melt = 1, dalb_mlt = -0.075, dalb_mltv = -0.1,
 * dalb_mlti = -0.15 (source/ice_shortwave.F90:709-716: local parameters that shadow the namelist variable); i0vis = 0.70 (:1079);
 * warmice = 0.68, coldice = 0.70, warmsnow = 0.77, coldsnow = 0.81 (:923-927).
 * Both calls are held bit for bit to a numpy restatement written from the Fortran (tests/nprad.py).  shortwave_ccsm3 with
 * compute_albedos, constant_albedos and absorbed_solar is PINNED to the reference's own compiled routines (oracle/ref/Makefile target
 * shortwave, tests/golden/ref_sw_c_*.npz): the restatement equals those records bit for bit on libm, and the device is compared with them
 * directly within four times the measured distance of its fixed-algorithm exp / atan from libm (at most 4.7e-16 of an array's largest
 * magnitude; tests/test_shortwave_ref.py, test_shortwave_ref_gpu.py).  **Parity unpinned** stay step_radiation's call order and zeroing,
 * the aggregation and scale_factor lines (the reference driver restates them), the stock scalar albocn path and evpk_prep_radiation.
 * Members (one struct of borrowed pointers; arrays (nx_block, ny_block[, ncat], nblocks) unless given):
 *   shortwave_dEdd, calc_Tsfc, heat_capacity (only 0, 1, 1 are accepted), albedo_constant (0 default / 1 'constant')
 *   ncat, ntrcr, ntrcr_dim, t (nt_Tsfc, nilyr, nslyr are read) as in evpk_thermo_args; puny (must be 1e-11)
 *   albicev, albicei, albsnowv, albsnowi, ahmax, snowpatch, albocn, awtvdr, awtidr, awtvdf, awtidf      the namelist's
 *   aicen, vicen, vsnon, trcrn                               in
 *   swvdr, swvdf, swidr, swidf, ocn_albedo2D                 in, 2-D; ocn_albedo2D may be NULL
 *   alvdrn, alidrn, alvdfn, alidfn, albicen, albsnon, fswsfcn, fswintn, fswthrun      out, per category, every cell
 *   Sswabsn (.., nslyr, ncat, ..), Iswabsn (.., nilyr, ncat, ..), fswpenln (.., nilyr+1, ncat, ..; may be NULL)    out, every cell
 *   coszen, alvdr, alidr, alvdf, alidf, albice, albsno, scale_factor                  out, 2-D, every cell
 * Nothing the call overwrites is copied up.
 *
 * evpk_prep_radiation: prep_radiation (source/ice_step_mod.F90:33-145), the rescaling in front of step_therm1 that drivers other than
 * AusCOM call, in one launch (k_prep_radiation).  drivers/auscom/CICE_RunMod.F90:332-338 compiles the call out: an AusCOM host does
 * NOT call it.  On every physical cell (land included, as in the reference): if aice > 0 and scale_factor > puny, scale_factor = netsw /
 * scale_factor with netsw built in the order of :87-90 (the order of the line that made scale_factor), else scale_factor = 1; fswfac =
 * scale_factor.  On the category list (physical, tmask, aicen > puny): fswsfcn, fswintn, fswthrun, the nilyr + 1 planes of fswpenln
 * where given and the layers of Sswabsn and Iswabsn are multiplied by that factor.  Ghost cells of every array, and land cells of the
 * category arrays, keep the caller's values.
 *   ncat, nilyr, nslyr, puny
 *   aice, aicen, swvdr, swvdf, swidr, swidf, alvdr_ai, alvdf_ai, alidr_ai, alidf_ai   in
 *   scale_factor, fswsfcn, fswintn, fswthrun, fswpenln (may be NULL), Sswabsn, Iswabsn      in / out
 *   fswfac                                                   out, physical cells
 * Both return 0; or 1 with evpk_last_error, before any copy, touching nothing: shortwave = 'dEdd'; calc_Tsfc = .false.; heat_capacity =
 * .false. (the zero-layer tail of absorbed_solar, :1218-1236); nilyr or nslyr outside 1..8; ncat outside 1..16; a tracer index beyond
 * ntrcr; puny != 1e-11; a missing pointer; a context of several ranks (nranks > 1) on which evpk_connect has not run.
 * x-slab ranks: neither call is collective -- a rank without a block column returns 0.
 * Out of scope: Delta-Eddington (run_dEdd) and everything it feeds: albpndn, apeffn, snowfracn, albpnd, apeff_ai; the tr_pond_topo
 * lines of the not-calc_Tsfc branch (:1482-1501); the remaining lines of coupling_prep: frzmlt_init, ocean_mixed_layer, albcnt, the
 * fpond / fresh lines, the _ai flux copies, scale_fluxes, sfcflux_to_ocn; the halo update of scale_factor (CICE_RunMod.F90:395) --
 * nothing here reads a ghost cell of it. */
#define EVPK_HAS_STEP_RADIATION 1
typedef struct {
    int32_t shortwave_dEdd, calc_Tsfc, heat_capacity, albedo_constant;
    int32_t ncat, ntrcr, ntrcr_dim;
    evpk_itd_tracers t;
    double puny;
    double albicev, albicei, albsnowv, albsnowi, ahmax, snowpatch, albocn, awtvdr, awtidr, awtvdf, awtidf;
    const double *aicen, *vicen, *vsnon, *trcrn;                              /* in */
    const double *swvdr, *swvdf, *swidr, *swidf, *ocn_albedo2D;               /* in; ocn_albedo2D may be NULL */
    double *alvdrn, *alidrn, *alvdfn, *alidfn, *albicen, *albsnon, *fswsfcn, *fswintn, *fswthrun;     /* out, per category, every cell */
    double *Sswabsn, *Iswabsn, *fswpenln;                                     /* out; fswpenln may be NULL */
    double *coszen, *alvdr, *alidr, *alvdf, *alidf, *albice, *albsno, *scale_factor;                  /* out, 2-D, every cell */
} evpk_rad_args;
typedef struct {
    int32_t ncat, nilyr, nslyr;
    double puny;
    const double *aice, *aicen, *swvdr, *swvdf, *swidr, *swidf, *alvdr_ai, *alvdf_ai, *alidr_ai, *alidf_ai;       /* in */
    double *scale_factor, *fswsfcn, *fswintn, *fswthrun, *fswpenln, *Sswabsn, *Iswabsn;       /* in / out; fswpenln may be NULL */
    double *fswfac;                                                           /* out */
} evpk_prep_rad_args;
int evpk_step_radiation(evpk_ctx *c, const evpk_rad_args *a);
int evpk_prep_radiation(evpk_ctx *c, const evpk_prep_rad_args *a);

/* The Delta-Eddington shortwave (kernel in csrc/evpk_dedd.hip, tables in csrc/evpk_dedd_tables.h, host layer in
 * csrc/evpk_api_column.hip): the scheme every ice_in of the
 * reference's own grids selects (shortwave = 'dEdd', reference/input_templates/{gx1,gx3,tp1,col}/ice_in).  evpk_step_radiation keeps
 * refusing shortwave_dEdd = 1; a Delta-Eddington host calls this instead.
 *
 * evpk_step_radiation_dedd: step_radiation (source/ice_step_mod.F90:1408-1451) on its calc_Tsfc / dEdd branch -- run_dEdd
 * (source/ice_shortwave.F90:1251-1577) with shortwave_dEdd_set_snow (:3782-3883), shortwave_dEdd_set_pond (:3893-3958), shortwave_dEdd
 * (:1607-2024), compute_dEdd (:2034-3261) and solution_dEdd (:3270-3772) -- and the albedo lines of coupling_prep that follow it at once
 * (drivers/auscom/CICE_RunMod.F90:503-548, :564-567, :582-586), in ONE launch (k_shortwave_dedd) for every category of every block: one
 * thread per cell that walks the categories in order.
 *   initialisation     on EVERY cell of the block arrays, ghost cells included (ice_step_mod.F90:1408-1423, ice_shortwave.F90:1428-1429,
 *                      :1744-1773): ZERO -- not the ocean albedo, which run_dEdd never writes -- in alvdrn, alidrn, alvdfn, alidfn,
 *                      albicen, albsnon, albpndn, apeffn, snowfracn, fswsfcn, fswintn, fswthrun, every layer of Sswabsn and Iswabsn and
 *                      every layer of fswpenln.  (The reference copies its whole work planes into apeffn and snowfracn, :1547, :1552;
 *                      set_snow and set_pond zero those planes first, :3838, :3936-3941, so a cell that is not listed holds zero)
 *   coszen             an IN / OUT 2-D plane: the caller passes what compute_coszen made (source/ice_orbital.F90:63-139; 0 where tmask is
 *                      false); shr_orb_decl and the libm sin / cos of ice_orbital.F90:130-132 stay on the host.  On a listed cell with
 *                      netsw > puny the kernel stores max(puny, coszen) back (:1814, :1869, :1922); everywhere else the plane keeps the
 *                      caller's value
 *   cell list          per category (:1406-1415): physical cells with aicen > puny AND tmask -- the stated departure of
 *                      evpk_thermo_vertical and of k_shortwave_ccsm3, kept so that every column kernel lists the same cells
 *   set_snow           (:3857-3880) hs = vsnon / aicen; fs = 1 under hs >= hs_min, min(hs / hs0, 1) under hs0 > puny; fT =
 *                      -min((Timelt - Tsfc) / dT_mlt - 1, 0) with the NAMELIST dT_mlt of the module (:134), not compute_albedos'
 *                      shadowing local; rsnw_nm = min(max(rsnw_nonmelt - R_snw rsnw_sig, rsnw_fresh), rsnw_mlt); rsnw = rsnw_nm +
 *                      (rsnw_mlt - rsnw_nm) fT, clamped likewise; rhosnw = rhos
 *   ponds              tr_pond_cesm (:1432-1448): fpn = trcrn(nt_apnd), hpn = trcrn(nt_hpnd); under hs >= hs_min and hs0 > puny asnow =
 *                      min(hs / hs0, 1), fpn = (1 - asnow) fpn, hpn = pndaspect fpn; apeffn = fpn.  No pond tracer (:1540-1550):
 *                      set_pond's 0.3 fT (1 - fs) (fT on dT_pnd = 1) feeds apeffn only, fpn = hpn = 0 go into the radiation.
 *                      tr_pond_lvl and tr_pond_topo are refused, as evpk_step_therm1 refuses them
 *   shortwave_dEdd     (:1762-1765) fnidr = swidr / (swidr + swidf) under swidr + swidf > puny, else 0; (:1812) netsw = swvdr + swidr +
 *                      swvdf + swidf in that order; hi = vicen / aicen; fi = (1 - fs) - fp (:1817); three passes -- bare ice under fi > 0
 *                      (with hs = 0, :1835), snow under fs > 0, pond under fp > puny -- each adds avdrl f and its like into the four
 *                      category albedos and the four-term awt* sum into albicen, albsnon, albpndn, left to right (:1848-1855, :1900-1907,
 *                      :1954-1961)
 *   compute_dEdd       band weights wghtns (:2602-2605); frsnw (:2612); the layer thicknesses dzk with both surface scattering layers
 *                      (:2618-2647); the R_ice / R_pnd adjustment of the ice and pond optical properties, both signs of each
 *                      (:2655-2721; uniform per call: computed on the host in this order); snow optical properties by linear
 *                      interpolation in the 32-radius table with both table ends (:2758-2785); pond layers (:2837-2841); the ice layers
 *                      with the kalg term in the lowest layer of band 1 (:2855-2886); ice under ponds and the pond-depth transition hpmin
 *                      <= hp <= hp0 (:2940-2986); albodr / albodf (:2992-2994); the interface fluxes dfdir / dfdif with their < puny -> 0
 *                      clamps (:3045-3051); the visible and near-infrared accumulations into fsfc, fint, fthru, Sabs, Iabs and fthrul
 *                      (-> fswpenln) with the km / kp indexing of the snow case (:3058-3186); the sums times the surface fraction
 *                      (:3197-3231)
 *   solution_dEdd      the statement functions alpha, agamm, n, u, el, taus, omgs, asys evaluated exactly as written (:3500-3508); mu0 =
 *                      max(coszen, 0.01) (:3535); the refracted mu0n (:3541); the trntdr > trmin cut-off (:3577); extins and trnlay under
 *                      max(exp_min, .) (:3597, :3607); the eight-point Gaussian recomputation of rdif / tdif with swt summed in the loop
 *                      (:3619-3639); the Fresnel layer at kfrsnl (:3649-3702); the downward (:3730-3738) and upward (:3754-3769) sweeps
 *   aggregation        every cell, categories in order (CICE_RunMod.F90:523-548): alvdf, alidf, alvdr, alidr and apeff_ai always; albice,
 *                      albsno, albpnd only under coszen > puny -- here the test decides, on the cell's coszen after the store above;
 *                      scale_factor as in :582-586.  alvdr_ai .. alidf_ai are plain copies (:564-567): the caller aliases them
 * Arithmetic: the Fortran's operation order, -ffp-contract=off; x**2 is x*x; min / max are a comparison and a select; sqrt is the IEEE one;
 * exp is dev_exp.  exp_min = exp(-argmax) with argmax = 10 a parameter (:1376, :1383), folded by the compiler with correct rounding: the
 * literal 4.5399929762484854e-05 = 0x3F07CD79B5647C9B, the double nearest to e^-10 (exact arithmetic: 2.6e-21 away; its neighbours 4.1e-21
 * and 9.4e-21).
 * Compiled in (csrc/evpk_dedd_tables.h names the lines): rsnw_tab, Qs_tab, ws_tab, gs_tab; the mean ice and pond optical properties; kw,
 * ww, gw; gauspt, gauswt; hi_ssl = 0.05, hs_ssl = 0.04, hpmin = 0.005, hp0 = 0.2, hs_min = 1e-4, rhoi = 917 (compute_dEdd's own), trmin =
 * 0.001, refindx = 1.31.  rhos is that of evpk_set_params.  evpk_dedd_table(name, out, n) reads any of them back.
 * Parity: run_dEdd and everything below it are PINNED to the reference's own compiled routines (oracle/ref/Makefile target shortwave,
 * tests/golden/ref_sw_d_*.npz): the restatement tests/npdedd.py, to which the call is held bit for bit, equals those records bit for bit
 * on libm, and the device is compared with them directly within four times the measured distance of its fixed-algorithm exp from libm
 * (at most 6.4e-14 of an array's largest magnitude; tests/test_shortwave_ref.py, test_shortwave_ref_gpu.py).
 * **Parity unpinned** stay step_radiation's call order and zeroing, the albedo aggregation / scale_factor lines of coupling_prep (the
 * reference driver restates them), aerosols and topographic ponds.
 * Members (one struct of borrowed pointers; arrays (nx_block, ny_block[, ncat], nblocks) unless given):
 *   calc_Tsfc, heat_capacity (only 1, 1 are accepted), tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_aero (a pond flag set here or in t counts)
 *   ncat, ntrcr, ntrcr_dim, t (nt_Tsfc, nt_apnd, nt_hpnd, nilyr, nslyr are read) as in evpk_thermo_args; puny (must be 1e-11)
 *   R_ice, R_pnd, R_snw, dT_mlt, rsnw_mlt, kalg, hs0, pndaspect, awtvdr, awtidr, awtvdf, awtidf      the namelist's (ice_init.F90:289-304)
 *   aicen, vicen, vsnon, trcrn, swvdr, swvdf, swidr, swidf   in
 *   coszen                                                   in / out, 2-D
 *   alvdrn, alidrn, alvdfn, alidfn, albicen, albsnon, fswsfcn, fswintn, fswthrun, albpndn, apeffn, snowfracn      out, per category, every cell
 *   Sswabsn (.., nslyr, ncat, ..), Iswabsn (.., nilyr, ncat, ..), fswpenln (.., nilyr+1, ncat, ..; may be NULL)    out, every cell
 *   alvdr, alidr, alvdf, alidf, albice, albsno, scale_factor, albpnd, apeff_ai        out, 2-D, every cell
 * Nothing the call overwrites is copied up.
 * Returns 0; or 1 with evpk_last_error, before any copy, touching nothing: calc_Tsfc = .false.; heat_capacity = .false.; tr_aero;
 * tr_pond_lvl; tr_pond_topo; tr_pond_cesm without nt_apnd / nt_hpnd; nilyr or nslyr outside 1..8; ncat outside 1..16; a tracer index
 * beyond ntrcr; puny != 1e-11; dT_mlt <= 0; a missing pointer (fswpenln may be NULL); a context of several ranks (nranks > 1) on which
 * evpk_connect has not run.  x-slab ranks: the call is not collective -- a rank without a block column returns 0.
 * Out of scope: level-ice and topographic ponds (dhsn, ffracn, :1450-1539); aerosols (aero_mp, :1775-1798 and the tr_aero blocks of
 * compute_dEdd); the zero-layer tail (:3240-3259); compute_coszen; albcnt; the rest of coupling_prep. */
#define EVPK_HAS_STEP_RADIATION_DEDD 1
typedef struct {
    int32_t calc_Tsfc, heat_capacity, tr_pond_cesm, tr_pond_lvl, tr_pond_topo, tr_aero;
    int32_t ncat, ntrcr, ntrcr_dim;
    evpk_itd_tracers t;
    double puny;
    double R_ice, R_pnd, R_snw, dT_mlt, rsnw_mlt, kalg, hs0, pndaspect, awtvdr, awtidr, awtvdf, awtidf;
    const double *aicen, *vicen, *vsnon, *trcrn;                              /* in */
    const double *swvdr, *swvdf, *swidr, *swidf;                              /* in */
    double *coszen;                                                           /* in / out */
    double *alvdrn, *alidrn, *alvdfn, *alidfn, *albicen, *albsnon, *fswsfcn, *fswintn, *fswthrun;     /* out, per category, every cell */
    double *Sswabsn, *Iswabsn, *fswpenln;                                     /* out; fswpenln may be NULL */
    double *alvdr, *alidr, *alvdf, *alidf, *albice, *albsno, *scale_factor;  /* out, 2-D, every cell */
    double *albpndn, *apeffn, *snowfracn;                                     /* out, per category, every cell */
    double *albpnd, *apeff_ai;                                                /* out, 2-D, every cell */
} evpk_dedd_args;
int evpk_step_radiation_dedd(evpk_ctx *c, const evpk_dedd_args *a);
int evpk_dedd_table(const char *name, double *out, int32_t n);

/* Level-ice melt ponds (tr_pond_lvl): the pond scheme every ice_in of the reference's own grids selects, with shortwave = 'dEdd', tr_lvl
 * and frzpnd = 'hlid' (reference/input_templates/{gx1,gx3,tp1,col}/ice_in).  evpk_step_therm1 and evpk_step_radiation_dedd keep refusing
 * tr_pond_lvl; a host on that scheme calls the two entry points below, which do everything their parents do and run
 *
 * evpk_step_therm1_lvl: compute_ponds_lvl with brine_permeability (source/ice_meltpond_lvl.F90:79-404) in the place of
 * compute_ponds_cesm, per category at the reference's call site (source/ice_step_mod.F90:623-642; the LVL instantiations of
 * k_therm1_merge, csrc/evpk_therm1s.hip), rfrac = rfracmin + (rfracmax - rfracmin) aicen, on the state thermo_vertical left:
 *   before the list    ffracn = 0 on EVERY cell of the block arrays, ghost cells and land included (:175-181); volpn = hpnd aicen alvl apnd
 *   cell list          the routine's own (:187-196): physical cells with aicen alvl > puny**2, AND tmask (the departure of every column
 *                      kernel here).  No aicen > puny test: it can list a cell that the thermodynamics does not
 *   on listed cells    hi < hi_min removes the pond and the lid (:206-215); the melt-water line dvn (:228-230); frzpnd = 0 'cesm': Tp =
 *                      Timelt - Td, dvn = dvn - volpn (1 - exp(rexp dTs / Tp)) (:233-236); frzpnd = 1 'hlid' (:238-267): hlid = ipnd; with
 *                      dvn == 0 and Ts = Tair - Tffresh < 0 the Stefan growth bdt = -2 Ts kice dt / (rhoi Lfresh), dhlid = sqrt(bdt) / 2
 *                      from open water or bdt / (2 hlid) on an existing lid, clamped by hpnd rhofresh / rhoi; with Ts >= 0 dhlid = 0; with
 *                      dvn /= 0 the lid melts by max(fsurfn dt / (rhoi Lfresh), 0) and, where hs - dhsn < puny (snow-free pond ice),
 *                      ffracn = 1 or, under fsurfn > puny, min(-dhlid rhoi Lfresh / (dt fsurfn), 1); dvn = dvn - dhlid alid rhoi / rhofresh;
 *                      volpn <= 0 (:274-277); existing ponds under apondn aicen > puny, new ponds under alvl aicen > 10 puny, else run-off
 *                      (:279-294); the freeboard limit hpondn <= ((rhow - rhoi) hi - rhos hs) / rhofresh (:297), which zeroes pond and
 *                      lid where it is not positive (:303-308); the drainage (:316-331) under hpondn > 0 and dpscale > puny -- ktherm is 1
 *                      here, evpk_thermo_vertical refuses anything else: calculate_Tin_from_qin under l_brine
 *                      (source/ice_therm_shared.F90:62-90), Sbr, phi with phi < 0.05 impermeable, perm = 3e-8 minval(phi)**3, drain =
 *                      perm pressure_head dt / (viscosity_dyn hi) dpscale, and the area and depth update after it; the nilyr enthalpy and
 *                      nilyr salinity planes are read only behind that test; the reload (:339-341): hpnd, apnd = apondn / (aicen alvl),
 *                      ipnd only under 'hlid'
 * evpk_step_radiation_dedd_lvl: the tr_pond_lvl block of run_dEdd (source/ice_shortwave.F90:1450-1514) in the place of the tr_pond_cesm
 * lines, on the list of k_shortwave_dedd (its LVL instantiations, csrc/evpk_dedd.hip): ipn = alvl apnd ipnd; dhs = dhsn, initialised to
 * hsn - fsnow dt where ipn > puny, dhs < puny and fsnow dt > hs_min, reset to 0 where ipn spn < puny (spn = hsn - dhs), both steps
 * skipped under linitonly, stored back into dhsn on the listed cells; fpn = apnd alvl, hpn = hpnd; fpn = (1 - ffracn) fpn; the taper
 * (1 - min(spn / hs1, 1)) under dhs > puny, spn >= puny, hs1 > puny; the infiltration under hp > puny: rp = rhofresh hp / (rhofresh hp +
 * rhos hs), rp < p15 hides the pond, otherwise tmp = max(0, sign(1, hp - hmx)), hp, and hsn = hs - hp fpn (1 - tmp) -- the modified hsn is
 * what shortwave_dEdd then receives; fpn = 0 under hpn < hpmin; fsn = min(fsn, 1 - fpn); apeffn = fpn; snowfracn = fsn.
 * Operation order: the Fortran's; min / max are a comparison and a select; sign is copysign-exact; x**3 is x*x*x; exp is dev_exp; sqrt is
 * the IEEE one.  Compiled in: Td = 2, rexp = 0.01 (source/ice_meltpond_lvl.F90:167-169); viscosity_dyn = 1.79e-3, kice = 2.03, gravit =
 * 9.80616, depressT = 0.054, cp_ocn = 4218, Tffresh = 273.15, rhofresh = 1000, Timelt = 0 (drivers/cice/ice_constants.F90:42, :71, :36,
 * :31, :29, :50, :45, :54); the permeability's 3e-8, 1e-3 and 0.05 (source/ice_meltpond_lvl.F90:393-402); hs_min = 1e-4
 * (drivers/auscom/ice_constants.F90:91), hpmin = 0.005 (source/ice_shortwave.F90:143), p15 = 0.15 (drivers/cice/ice_constants.F90:139).
 * rhoi, rhos, rhow are evpk_set_params'; cp_ice, Lfresh, puny come from tv.k.
 * Both calls are held bit for bit to a numpy restatement written from the Fortran (tests/nppondlvl.py, on top of tests/nptherm1s.py and
 * tests/npdedd.py).  The tr_pond_lvl block of run_dEdd is PINNED with run_dEdd (tests/golden/ref_sw_v_*.npz, initonly absent and .true.),
 * and compute_ponds_lvl with brine_permeability is pinned on the CPU (ref_sw_p_*.npz; the restatement alone -- the device has no entry
 * point for it alone, and the AusCOM build's cp_ocn = 3989.24495292815 is handed to the restatement where the device carries 4218).
 * **Parity unpinned** stays evpk_step_therm1_lvl as a whole, with step_therm1 and thermo_vertical.
 * evpk_pond_lvl_args: what the two routines hand each other, and the scheme's own namelist --
 *   dhsn     per category: the shortwave reads and writes it (listed cells), the thermodynamics reads it
 *   ffracn   per category: the thermodynamics writes it on every cell, the shortwave reads it
 *   Tair     2-D, in, read by the thermodynamics only (may be NULL for the shortwave)
 *   fsnow    2-D, in, read by the shortwave only (may be NULL for the thermodynamics, whose own fsnow is tv.fsnow)
 *   dpscale, hs1 (source/ice_init.F90:299-300: defaults 1, 0.03; the shipped ice_in set dpscale = 1e-3), dt -- the shortwave's, read by it only; frzpnd 0 'cesm' / 1 'hlid'; nt_ipnd; linitonly (the
 *   shortwave's initonly).  nt_alvl, nt_apnd, nt_hpnd are those of the evpk_itd_tracers of the parent's struct.
 * evpk_step_therm1_lvl needs frain.  Host arrays and device pointers both work, staged once with the parent's.
 * Both return what their parents return; or 1 with evpk_last_error, before any copy, touching nothing: tr_pond_lvl unset; nt_alvl,
 * nt_apnd, nt_hpnd or nt_ipnd missing or beyond ntrcr; frzpnd outside 0..1; a missing dhsn, ffracn, Tair (thermodynamics) or fsnow
 * (shortwave); pndaspect <= 0 or frain missing (thermodynamics); dt <= 0 (shortwave); everything the parent refuses (tr_pond_cesm set
 * beside tr_pond_lvl included).  x-slab ranks: not collective, as the parents are not.
 * Out of scope: tr_pond_topo, ktherm = 2, the pond restart records. */
#define EVPK_HAS_POND_LVL 1
typedef struct {
    double *dhsn, *ffracn;                                                    /* in / out, per category */
    const double *Tair, *fsnow;                                               /* in, 2-D */
    double dpscale, hs1, dt;
    int32_t frzpnd, nt_ipnd, linitonly;
} evpk_pond_lvl_args;
int evpk_step_therm1_lvl(evpk_ctx *c, const evpk_therm1_args *a, const evpk_pond_lvl_args *p, int32_t stop[5]);
int evpk_step_radiation_dedd_lvl(evpk_ctx *c, const evpk_dedd_args *a, const evpk_pond_lvl_args *p);

/* the elastic-anisotropic-plastic rheology, eap(dt) (source/ice_dyn_eap.F90:66-486; kdyn = 2,
 * ice_step_mod.F90:1118).  eap is evp with another stress: evp_prep1/2, stepu, the velocity halo, evp_finish are shared
 * (:79-80), stress_eap (:1052-1467) with update_stress_rdg (:1474-1658) takes the place of stress, stepa (:1664-1787, with
 * calc_ffrac :1795-1864) evolves the structure tensor every tenth subcycle, and there is no stress fold at the end.
 *
 * evpk_eap_init switches the context to EAP: every later evpk_run / evpk_subcycle runs the eap loop.  It takes the six
 * lookup tables init_eap builds on the host (:555-619; module arrays s11r ... s22s(nx_yield, ny_yield, na_yield), :36-39) and
 * sets the structure tensor to isotropic (a11 = 1/2, a12 = 0, :529-551) as init_eap does.
 * evpk_eap_upload moves a11_1..4, a12_1..4 (the prognostic EAP state: restart, read_restart_eap :1908-2010) to the device
 * (members that are NULL stay as they are); evpk_eap_download brings back any non-NULL member: physical cells and the N / E
 * ghost T cells, as the reference computes them.
 * sin, cos and atan2 inside update_stress_rdg / calc_ffrac are fixed algorithms (csrc/evpk_fmath.h, within 1-2 ulp of libm):
 * the table indices depend on the last bit of an angle, so results agree with another math library except where an index
 * falls on the other side of a table cell -- as between any two compilers of the reference. */
typedef struct {
    double *a11_c[4], *a12_c[4];      /* a11_1..4, a12_1..4: structure tensor at the corners ne, nw, sw, se (ice_dyn_eap.F90:40-41) */
    double *a11, *a12;                /* out: cell means (history, :55-56) */
    double *e11, *e12, *e22;          /* out: strain rate tensor (:47-49) */
    double *yieldstress11, *yieldstress12, *yieldstress22;      /* out (:50-52) */
    double *s11, *s12, *s22;          /* out: stress tensor (:53-55) */
} evpk_eap_state;
int evpk_eap_init(evpk_ctx *c, int32_t nx_yield, int32_t ny_yield, int32_t na_yield, const double *s11r, const double *s12r,
                  const double *s22r, const double *s11s, const double *s12s, const double *s22s);
int evpk_eap_upload(evpk_ctx *c, const evpk_eap_state *st);
int evpk_eap_download(evpk_ctx *c, evpk_eap_state *st);

/* The dynamics records of the reference's binary restart (source/ice_restart_driver.F90:122-176 dumpfile, :295-412
 * restartfile; io_binary/ice_restart.F90:641-684): uvel, vvel, strocnxT, strocnyT, stressp_1,3,2,4, stressm_1,3,2,4,
 * stress12_1,3,2,4, iceumask as real 0/1 -- 17 Fortran sequential unformatted records of the (nx_global, ny_global)
 * real*8 array, big-endian under the production flags.  Written from / read into the state resident on the device (one
 * rank; a multi-rank host gathers through its own path as the reference does).  evpk_restart_read fills the ghost
 * cells as restartfile does (halo by field location and type, then the twelve ice_HaloUpdate_stress pairings on
 * tripole grids, :370-395) and leaves the context as after evpk_upload: evpk_upload(in, NULL) may follow.
 * byte_offset: where the first of the 17 records starts in the file (they are consecutive in this library's own files;
 * in a full CICE restart the radiation fields sit between vvel and strocnxT, so that file goes through the host). */
int evpk_restart_write(evpk_ctx *c, const char *path, int32_t append, int32_t big_endian);
int evpk_restart_read(evpk_ctx *c, const char *path, int64_t byte_offset, int32_t big_endian);

/* Profiling aid: nrep device-to-device copies of one scratch pair plane with the hot kernel's access
 * shape (16 B per lane, coalesced).  Each moves exactly (nxl+2)*(nyl+2)*16 bytes each way: a known
 * byte count in the PMC trace to calibrate FETCH_SIZE / WRITE_SIZE (MI355X_MICROARCH.md, HBM). */
/* Each call also runs nrep copies of EVPK_CALIB_BIG_BYTES from one buffer to another (kernel k_calib_copy_big): both far
 * larger than the 256 MiB Infinity Cache, the byte count the FETCH_SIZE correction is checked against. */
#define EVPK_CALIB_BIG_BYTES (1ull << 30)
int evpk_calibrate(evpk_ctx *c, int32_t nrep);
int evpk_destroy(evpk_ctx *c);

/* Optional: page-lock a host array the caller keeps for the life of the run (CICE's module arrays of ice_state /
 * ice_flux / ice_grid, ice_state.F90 / ice_flux.F90) and map it into the device address space.  evpk_upload /
 * evpk_download / evpk_run then read and write such arrays in place over PCIe instead of staging them, and a download
 * touches only the cells it delivers.  Arrays that were not registered keep working (staged copies).  Unpin before the
 * memory is freed.  Returns 0 on success; non-zero if the range overlaps a live registration or the runtime refuses.
 * The library moves an array in place ONLY if all of it lies inside a range registered here (and not yet released) or
 * handed out by evpk_host_alloc -- it keeps its own table and never trusts a registration it did not make.  The pages
 * of a registered range are advised MADV_NOHUGEPAGE and mlock'ed (best effort; EVPK_PIN_HARDEN=0 skips both):
 * hipHostRegister mirrors the caller's pages through MMU notifiers, it does not hard-pin them.
 * evpk_host_alloc / evpk_host_free: page-locked memory allocated and pinned BY THE DRIVER (hipHostMalloc), mapped into
 * the device address space -- for a host that can choose where its arrays live (allocatable arrays, c_f_pointer).
 * evpk_host_is_mapped: 1 if [ptr, ptr + bytes) would be moved in place.
 * EVPK_VERIFY_DELIVERY=1 (diagnostic): every plane a download writes in place is delivered a second time through the
 * staged path and compared on the host; a difference fails the call with plane, block, cell and page in
 * evpk_last_error (=2: the caller's array is repaired and the event counted, evpk_stats.delivery_bad). */
/* Arrays that already live in DEVICE memory (a host model whose fields are resident on the GPU: OpenMP target /
 * OpenACC use_device pointers, hipMalloc) may be passed wherever a host array is expected: the library detects them
 * (hipPointerGetAttributes) and gathers / scatters them in place, no PCIe transfer at all. */
int evpk_pin_host(void *ptr, size_t bytes);
int evpk_unpin_host(void *ptr);
int evpk_host_alloc(size_t bytes, void **out);
int evpk_host_free(void *ptr);
int evpk_host_is_mapped(const void *ptr, size_t bytes);
const char *evpk_last_error(const evpk_ctx *c);  /* c may be NULL: error of the last failed evpk_create */

/* Host-only description of this rank's halo exchange (no GPU needed): neighbours in the
 * slab ring and the fold partner layout.  Used by the world_size-2 CPU tests.
 *   out[0] = west rank (-1 none), out[1] = east rank (-1 none),
 *   out[2] = first global column i0, out[3] = last global column i1,
 *   out[4] = columns per rank used for the tripole all-gather (max slab width) */
int evpk_slab_layout(int32_t nx_global, int32_t nranks, int32_t rank, int32_t ew_boundary,
                     int32_t i0, int32_t i1, int32_t out[5]);

#ifdef __cplusplus
}
#endif
#endif
