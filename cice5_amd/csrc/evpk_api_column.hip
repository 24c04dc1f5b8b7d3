// evpk_api_column.hip -- the host layer of the column physics: the entry points of include/evpk.h whose kernels take one thread per cell of
// the caller's block arrays and walk the categories.  Included by evpk_api.hip behind the step_therm2 section; not a translation unit.
//   evpk_thermo_vertical                                      k_thermo_vertical (evpk_therm1.hip)
//   evpk_step_therm1, evpk_step_therm1_lvl                    k_therm1_open, evpk_thermo_vertical, k_therm1_merge (evpk_therm1s.hip)
//   evpk_step_radiation, evpk_prep_radiation                  k_shortwave_ccsm3, k_prep_radiation (evpk_rad.hip)
//   evpk_step_radiation_dedd, evpk_step_radiation_dedd_lvl    k_shortwave_dedd (evpk_dedd.hip)
//   evpk_dedd_table                                           the tables of evpk_dedd_tables.h, no context
// Relies on evpk_api.hip for the context, FAIL / HIPCHK / RANKS_ENTRY, HostArr / OptArr / any_missing / stage_in / stage_out, grow,
// with_bool / with_ncat / with_layers and launch_blocks.
// Every entry point states its caller arrays ONCE, in the list it hands to stage_in; any_missing on that same list is the NULL check, made
// where the checks have always made it.  An array the caller may leave out is an OptArr: where a flag makes it necessary, the refusal that
// names it stands among the checks.  The list is built before the checks: its sizes need the context and ncat only, and are not used
// before ncat has passed.

// What every entry point begins with: no context is 1 without a message, the stop record (where there is one) starts out zero,
// RANKS_ENTRY, and `given` -- the argument structs and the stop record -- must be there.
#define COLUMN_ENTRY(c, who, stop, given)                                  \
    do {                                                                   \
        if (!(c)) return 1;                                                \
        for (int _q = 0; (stop) && _q < 5; _q++) (stop)[_q] = 0;           \
        RANKS_ENTRY(c, who);                                               \
        if (!(given)) FAIL(c, "%s: a required argument is missing", who);  \
    } while (0)
static int32_t *const NO_STOP = nullptr;

// the refusals several entry points share, each in the place its entry point has always made it
static int flags_check(evpk_ctx *c, const char *who, int calc_Tsfc, int heat_capacity) {
    if (calc_Tsfc != 1) FAIL(c, "%s: calc_Tsfc = .false. is not supported", who);
    if (heat_capacity != 1) FAIL(c, "%s: heat_capacity = .false. (zero-layer) is not supported", who);
    return 0;
}
static int layers_check(evpk_ctx *c, const char *who, int nilyr, int nslyr, int maxl) {
    if (nilyr < 1 || nslyr < 1 || nilyr > maxl || nslyr > maxl) FAIL(c, "%s: nilyr = %d, nslyr = %d not in 1..%d", who, nilyr, nslyr, maxl);
    return 0;
}
static int ncat_check(evpk_ctx *c, const char *who, int ncat) {
    if (ncat < 1 || ncat > MAXCAT) FAIL(c, "%s: ncat = %d not in 1..%d", who, ncat, MAXCAT);
    return 0;
}
static int Tsfc_check(evpk_ctx *c, const char *who, int ntrcr, int ntrcr_dim, int nt_Tsfc) {
    if (ntrcr < 1 || ntrcr_dim < ntrcr || nt_Tsfc < 1 || nt_Tsfc > ntrcr)
        FAIL(c, "%s: nt_Tsfc = %d lies beyond ntrcr = %d (ntrcr_dim = %d)", who, nt_Tsfc, ntrcr, ntrcr_dim);
    return 0;
}
static int puny_check(evpk_ctx *c, const char *who, double puny) {
    if (puny != 1.0e-11) FAIL(c, "%s: puny = %g: the device code is built with 1e-11", who, puny);
    return 0;
}

// ---- thermo_vertical (source/ice_therm_vertical.F90:79-531), BL99, for every category of every block in one launch (kernel in
// evpk_therm1.hip) ----
// The arrays evpk_thermo_vertical and evpk_step_therm1 have in common, into d: a ThermoArgs, or the evpk_thermo_args of device pointers
// that step_therm1 passes on.  fbot, Tbot, shcoef and lhcoef are the caller's to add: inputs of the one, made by the other.
// (sss is not staged: ktherm = 1 does not read it; the fifteen outputs are not copied up)
template <class D> static std::vector<HostArr> thermo_arrays(const evpk_thermo_args &a, size_t N, size_t n3, D &d) {
    const evpk_itd_tracers &t = a.t;
    return {{a.aicen, n3, &d.aicen, true}, {a.vicen, n3, &d.vicen, true}, {a.vsnon, n3, &d.vsnon, true}, {a.trcrn, n3 * a.ntrcr_dim, &d.trcrn, true},
            {a.flw, N, &d.flw, false}, {a.potT, N, &d.potT, false}, {a.Qa, N, &d.Qa, false}, {a.rhoa, N, &d.rhoa, false}, {a.fsnow, N, &d.fsnow, false},
            {a.fswsfcn, n3, &d.fswsfcn, true}, {a.fswintn, n3, &d.fswintn, true}, {a.Sswabsn, n3 * t.nslyr, &d.Sswabsn, true},
            {a.Iswabsn, n3 * t.nilyr, &d.Iswabsn, true}, OptArr(t.tr_pond_topo ? a.fpond : nullptr, N, &d.fpond, true),
            {a.mlt_onset, N, &d.mlt_onset, true}, {a.frz_onset, N, &d.frz_onset, true},
            {a.flwoutn, n3, &d.flwoutn, true, false}, {a.evapn, n3, &d.evapn, true, false}, {a.freshn, n3, &d.freshn, true, false},
            {a.fsaltn, n3, &d.fsaltn, true, false}, {a.fhocnn, n3, &d.fhocnn, true, false}, {a.fsensn, n3, &d.fsensn, true, false},
            {a.flatn, n3, &d.flatn, true, false}, {a.fsurfn, n3, &d.fsurfn, true, false}, {a.fcondtopn, n3, &d.fcondtopn, true, false},
            {a.melttn, n3, &d.melttn, true, false}, {a.meltsn, n3, &d.meltsn, true, false}, {a.meltbn, n3, &d.meltbn, true, false},
            {a.congeln, n3, &d.congeln, true, false}, {a.snoicen, n3, &d.snoicen, true, false}, {a.dsnown, n3, &d.dsnown, true, false}};
}

// what evpk_thermo_vertical refuses (arr: its arrays, or those of them evpk_step_therm1 needs from its caller)
static int thermo_check(evpk_ctx *c, const char *who, const evpk_thermo_args *a, const std::vector<HostArr> &arr) {
    const evpk_itd_tracers &t = a->t;
    if (a->ktherm != 1) FAIL(c, "%s: ktherm = %d: only ktherm = 1 (BL99) is supported", who, a->ktherm);
    if (flags_check(c, who, a->calc_Tsfc, a->heat_capacity)) return 1;
    if (a->l_brine != 1) FAIL(c, "%s: l_brine = .false. (fresh ice) is not supported", who);
    if (a->conduct != 0 && a->conduct != 1) FAIL(c, "%s: conduct = %d not 0 (MU71) or 1 (bubbly)", who, a->conduct);
    if (any_missing(arr) || !a->sss || a->ntrcr < 1 || a->ntrcr_dim < a->ntrcr) FAIL(c, "%s: a required argument is missing", who);
    if (!c->connected) FAIL(c, "%s: the context is not connected yet (evpk_connect)", who);
    if (!c->have_params) FAIL(c, "%s: evpk_set_params has not been called (rhow, rhoi, rhos)", who);
    if (!(a->dt > 0.0)) FAIL(c, "%s: dt = %g", who, a->dt);
    if (ncat_check(c, who, a->ncat)) return 1;
    if (a->ntrcr > RG_MAXT) FAIL(c, "%s: ntrcr = %d exceeds %d", who, a->ntrcr, RG_MAXT);
    if (puny_check(c, who, a->k.puny)) return 1;
    if (t.nt_Tsfc < 1 || t.nt_qice < 1 || t.nt_qsno < 1 || a->nt_sice < 1) FAIL(c, "%s: nt_Tsfc, nt_qice, nt_qsno and nt_sice are required", who);
    if (layers_check(c, who, t.nilyr, t.nslyr, T1_MAXL)) return 1;
    if (t.nt_Tsfc > a->ntrcr || t.nt_qice + t.nilyr - 1 > a->ntrcr || t.nt_qsno + t.nslyr - 1 > a->ntrcr || a->nt_sice + t.nilyr - 1 > a->ntrcr)
        FAIL(c, "%s: a tracer index lies beyond ntrcr = %d", who, a->ntrcr);
    if (t.tr_pond_topo && (!a->fpond || t.nt_apnd < 1 || t.nt_hpnd < 1 || t.nt_apnd > a->ntrcr || t.nt_hpnd > a->ntrcr))
        FAIL(c, "%s: tr_pond_topo needs fpond, nt_apnd and nt_hpnd", who);
    if (c->nblocks >= 65536) FAIL(c, "%s: %d blocks exceed the stop key", who, c->nblocks);
    return 0;
}

extern "C" int evpk_thermo_vertical(evpk_ctx *c, const evpk_thermo_args *a, int32_t stop[5]) {
    COLUMN_ENTRY(c, "evpk_thermo_vertical", stop, a && stop);
    const evpk_itd_tracers &t = a->t;
    ThermoArgs T{};
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb, n3 = N * a->ncat;
    std::vector<HostArr> arr = thermo_arrays(*a, N, n3, T);
    arr.insert(arr.end(), {{a->fbot, N, &T.fbot, false}, {a->Tbot, N, &T.Tbot, false}, {a->shcoef, n3, &T.shcoef, false}, {a->lhcoef, n3, &T.lhcoef, false}});
    if (thermo_check(c, "evpk_thermo_vertical", a, arr)) return 1;
    if (!c->nblocks) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    T.ncat = a->ncat; T.ntrcr_dim = a->ntrcr_dim; T.nxb = c->nxb; T.nyb = c->nyb; T.nilyr = t.nilyr; T.nslyr = t.nslyr;
    T.nt_Tsfc = t.nt_Tsfc; T.nt_qice = t.nt_qice; T.nt_qsno = t.nt_qsno; T.nt_sice = a->nt_sice; T.nt_apnd = t.nt_apnd; T.nt_hpnd = t.nt_hpnd;
    T.tr_pond_topo = t.tr_pond_topo ? 1 : 0; T.conduct = a->conduct;
    T.dt = a->dt; T.yday = a->yday; T.min_salin = a->min_salin; T.puny = a->k.puny; T.rhoi = c->p.rhoi; T.rhos = c->p.rhos; T.rhow = c->p.rhow;
    T.cp_ice = a->k.cp_ice; T.Lfresh = a->k.Lfresh; T.hs_min = a->k.hs_min; T.Tmin = a->k.Tmin; T.salinity = a->k.ice_ref_salinity;
    if (stage_in(c, arr, true)) return 1;
    if (!c->itd_key) HIPCHK(c, hipMalloc(&c->itd_key, sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->itd_key, 0xff, sizeof(unsigned long long), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    int rc = 0;
    with_layers(a->ncat, t.nilyr, t.nslyr, [&](auto... S) { rc = launch_blocks(c, k_thermo_vertical<decltype(S)::value...>, T, c->itd_key); });
    if (rc) return 1;
    unsigned long long key = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&key, c->itd_key, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    if (stage_out(c, arr)) return 1;
    if (key == ~0ull) return 0;
    const int seq = (int)((key >> 32) & 0xff), ns = t.nslyr, nl = t.nilyr;
    const size_t o = (size_t)(key & 0xffffffffull);
    stop[0] = seq < ns ? T1_STOP_TSN_HIGH : seq < 2 * ns ? T1_STOP_TSN_LOW : seq < 2 * ns + 3 * nl ? T1_STOP_SALIN + (seq - 2 * ns) % 3
              : seq == 2 * ns + 3 * nl ? T1_STOP_NITER : T1_STOP_ENERGY;
    stop[1] = (int32_t)(key >> 48) + 1; stop[2] = (int32_t)((key >> 40) & 0xff) + 1; stop[3] = (int32_t)(o % c->nxb) + 1; stop[4] = (int32_t)(o / c->nxb) + 1;
    return EVPK_THERMO_STOP;
}

// what the two level-ice pond entry points refuse beyond their parents
static int pond_lvl_check(evpk_ctx *c, const char *who, const evpk_itd_tracers &t, int ntrcr, const evpk_pond_lvl_args *p) {
    const int nts[4] = {t.nt_alvl, t.nt_apnd, t.nt_hpnd, p->nt_ipnd};
    for (int nt : nts)
        if (nt < 1 || nt > ntrcr) FAIL(c, "%s: tr_pond_lvl without nt_alvl / nt_apnd / nt_hpnd / nt_ipnd in 1..ntrcr = %d", who, ntrcr);
    if (p->frzpnd < 0 || p->frzpnd > 1) FAIL(c, "%s: frzpnd = %d not 0 ('cesm') or 1 ('hlid')", who, p->frzpnd);
    if (!p->dhsn || !p->ffracn) FAIL(c, "%s: tr_pond_lvl needs dhsn and ffracn", who);
    return 0;
}

// ---- step_therm1 (source/ice_step_mod.F90:154-733) in one call: k_therm1_open, k_thermo_vertical, k_therm1_merge (evpk_therm1s.hip) on
// state staged once ----
// p: the level-ice pond arguments of evpk_step_therm1_lvl, or null for evpk_step_therm1
static int therm1_run(evpk_ctx *c, const char *who, const evpk_therm1_args *a, const evpk_pond_lvl_args *p, int32_t stop[5]) {
    const evpk_thermo_args &v = a->tv;
    const evpk_itd_tracers &t = v.t;
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb, n3 = N * v.ncat;
    evpk_thermo_args x = v;                 // thermo_vertical's arguments on device pointers
    Therm1sArgs A{};
    double *d_opt[8] = {};                  // shcoef, lhcoef, strairxn, strairyn, Cdn_atm_ratio_n, Trefn, Qrefn, Urefn where the caller gives them
    double *d_fbot = nullptr, *d_Tbot = nullptr;
    double *const h_opt[8] = {const_cast<double *>(v.shcoef), const_cast<double *>(v.lhcoef), a->strairxn, a->strairyn, a->Cdn_atm_ratio_n, a->Trefn,
                              a->Qrefn, a->Urefn};
    double *const merged[T1S_NMERGE] = {a->strairxT, a->strairyT, a->Cdn_atm_ratio, a->fsurf, a->fcondtop, a->fsens, a->flat, a->fswabs, a->flwout, a->evap,
                                        a->Tref, a->Qref, a->Uref, a->fresh, a->fsalt, a->fhocn, a->fswthru, a->meltt, a->meltb, a->melts, a->congel, a->snoice};
    std::vector<HostArr> arr = thermo_arrays(v, N, n3, x);
    if (a->formdrag) FAIL(c, "%s: formdrag (neutral_drag_coeffs) is not supported", who);
    if (a->highfreq) FAIL(c, "%s: highfreq coupling is not supported", who);
    if (a->atmbndy_constant) FAIL(c, "%s: atmbndy = 'constant' (atmo_boundary_const) is not supported", who);
    if (a->fbot_xfer_Cdn_ocn) FAIL(c, "%s: fbot_xfer_type = 'Cdn_ocn' is not supported", who);
    if (!p && t.tr_pond_lvl) FAIL(c, "%s: tr_pond_lvl (compute_ponds_lvl) is not supported", who);
    if (p && !t.tr_pond_lvl) FAIL(c, "%s: tr_pond_lvl is not set", who);
    if (p && t.tr_pond_cesm) FAIL(c, "%s: tr_pond_cesm is set beside tr_pond_lvl", who);
    if (t.tr_pond_topo) FAIL(c, "%s: tr_pond_topo (compute_ponds_topo) is not supported", who);
    if (a->tr_aero) FAIL(c, "%s: aerosol tracers (tr_aero, update_aerosol) are not supported", who);
    if (thermo_check(c, who, &v, arr)) return 1;
    if (a->natmiter < 1) FAIL(c, "%s: natmiter = %d", who, a->natmiter);
    arr.insert(arr.end(), {          // (arrays a call only writes are not copied up; ffracn is written on every cell)
        OptArr(v.fbot, N, &d_fbot, true, false), OptArr(v.Tbot, N, &d_Tbot, true, false),
        {a->aice, N, &A.aice, false}, {a->frzmlt, N, &A.frzmlt, false}, {a->sst, N, &A.sst, false}, {a->Tf, N, &A.Tf, false},
        {a->strocnxT, N, &A.strocnxT, false}, {a->strocnyT, N, &A.strocnyT, false}, {a->uatm, N, &A.uatm, false}, {a->vatm, N, &A.vatm, false},
        {a->wind, N, &A.wind, false}, {a->zlvl, N, &A.zlvl, false}, OptArr(t.tr_pond_cesm || p ? a->frain : nullptr, N, &A.frain, false),
        {a->fswthrun, n3, &A.fswthrun, false}, OptArr(a->tr_FY ? a->lmask_n : nullptr, N, &A.lmask_n, false),
        OptArr(a->tr_FY ? a->lmask_s : nullptr, N, &A.lmask_s, false),
        {a->Cdn_atm, N, &A.Cdn_atm, true}, {a->rside, N, &A.rside, true, false}, {a->aice_init, N, &A.aice_init, true, false},
        {a->aicen_init, n3, &A.aicen_init, true, false}, {a->vicen_init, n3, &A.vicen_init, true, false},
        OptArr(p ? p->dhsn : nullptr, n3, &A.dhsn, false), OptArr(p ? p->ffracn : nullptr, n3, &A.ffracn, true, false),
        OptArr(p ? p->Tair : nullptr, N, &A.Tair, false)});
    for (int q = 0; q < 8; q++) arr.push_back(OptArr(h_opt[q], n3, &d_opt[q], true, false));
    for (int q = 0; q < T1S_NMERGE; q++) arr.push_back({merged[q], N, &A.m[q], true});
    if (any_missing(arr)) FAIL(c, "%s: a required argument is missing", who);
    if (a->tr_iage && (a->nt_iage < 1 || a->nt_iage > v.ntrcr)) FAIL(c, "%s: tr_iage without nt_iage in 1..ntrcr = %d", who, v.ntrcr);
    if (a->tr_FY && (a->nt_FY < 1 || a->nt_FY > v.ntrcr)) FAIL(c, "%s: tr_FY without nt_FY in 1..ntrcr = %d", who, v.ntrcr);
    if (a->tr_FY && (!a->lmask_n || !a->lmask_s)) FAIL(c, "%s: tr_FY needs lmask_n and lmask_s", who);
    if (t.tr_pond_cesm && (t.nt_apnd < 1 || t.nt_hpnd < 1 || t.nt_apnd > v.ntrcr || t.nt_hpnd > v.ntrcr))
        FAIL(c, "%s: tr_pond_cesm without nt_apnd / nt_hpnd in 1..ntrcr = %d", who, v.ntrcr);
    if (t.tr_pond_cesm && !a->frain) FAIL(c, "%s: tr_pond_cesm needs frain", who);
    if (t.tr_pond_cesm && !(a->pndaspect > 0.0)) FAIL(c, "%s: pndaspect = %g", who, a->pndaspect);
    if (p) {
        if (pond_lvl_check(c, who, t, v.ntrcr, p)) return 1;
        if (!p->Tair) FAIL(c, "%s: tr_pond_lvl needs Tair", who);
        if (!a->frain) FAIL(c, "%s: tr_pond_lvl needs frain", who);
        if (!(a->pndaspect > 0.0)) FAIL(c, "%s: pndaspect = %g", who, a->pndaspect);
    }
    if (!c->nblocks) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (stage_in(c, arr, true)) return 1;
    HIPCHK(c, grow(c, c->th1_pool, c->th1_pool_n, 8 * n3 + 2 * N));        // one pool, grown once
    for (int q = 0; q < 8; q++) if (!d_opt[q]) d_opt[q] = c->th1_pool + (size_t)q * n3;
    if (!d_fbot) d_fbot = c->th1_pool + 8 * n3;
    if (!d_Tbot) d_Tbot = c->th1_pool + 8 * n3 + N;
    x.fbot = d_fbot; x.Tbot = d_Tbot; x.shcoef = d_opt[0]; x.lhcoef = d_opt[1];
    x.sss = v.sss;                            // (not read: any non-null pointer passes the check)
    A.potT = x.potT; A.Qa = x.Qa; A.rhoa = x.rhoa; A.flw = x.flw;
    A.aicen = x.aicen; A.vicen = x.vicen; A.vsnon = x.vsnon; A.trcrn = x.trcrn;
    A.fbot = d_fbot; A.Tbot = d_Tbot;
    A.shcoef = d_opt[0]; A.lhcoef = d_opt[1]; A.strairxn = d_opt[2]; A.strairyn = d_opt[3]; A.Cdn_atm_ratio_n = d_opt[4]; A.Trefn = d_opt[5];
    A.Qrefn = d_opt[6]; A.Urefn = d_opt[7];
    A.fswsfcn = x.fswsfcn; A.fswintn = x.fswintn; A.flwoutn = x.flwoutn; A.evapn = x.evapn; A.freshn = x.freshn; A.fsaltn = x.fsaltn; A.fhocnn = x.fhocnn;
    A.fsensn = x.fsensn; A.flatn = x.flatn; A.fsurfn = x.fsurfn; A.fcondtopn = x.fcondtopn; A.melttn = x.melttn; A.meltsn = x.meltsn; A.meltbn = x.meltbn;
    A.congeln = x.congeln; A.snoicen = x.snoicen;
    A.ncat = v.ncat; A.ntrcr_dim = v.ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb; A.nilyr = t.nilyr; A.nslyr = t.nslyr; A.nt_Tsfc = t.nt_Tsfc;
    A.nt_qice = t.nt_qice; A.nt_qsno = t.nt_qsno; A.nt_apnd = t.nt_apnd; A.nt_hpnd = t.nt_hpnd; A.nt_iage = a->nt_iage; A.nt_FY = a->nt_FY;
    A.tr_iage = a->tr_iage ? 1 : 0; A.tr_FY = a->tr_FY ? 1 : 0; A.tr_pond_cesm = t.tr_pond_cesm ? 1 : 0; A.calc_strair = a->calc_strair ? 1 : 0;
    A.natmiter = a->natmiter;
    if (p) {
        A.nt_alvl = t.nt_alvl; A.nt_ipnd = p->nt_ipnd; A.nt_sice = v.nt_sice; A.frzpnd = p->frzpnd; A.dpscale = p->dpscale;
        A.Lfresh = v.k.Lfresh; A.cp_ice = v.k.cp_ice;
    }
    A.dt = v.dt; A.yday = v.yday; A.puny = v.k.puny; A.rhoi = c->p.rhoi; A.rhos = c->p.rhos; A.rhow = c->p.rhow; A.chio = a->chio;
    A.ustar_min = a->ustar_min; A.hi_min = a->hi_min; A.pndaspect = a->pndaspect; A.rfracmin = a->rfracmin; A.rfracmax = a->rfracmax;
    int rc = 0;
    with_ncat(v.ncat, [&](auto NC) { rc = launch_blocks(c, k_therm1_open<decltype(NC)::value>, A); });
    if (rc) return 1;
    // thermo_vertical on the staged arrays: its own staging finds device pointers and copies nothing
    rc = evpk_thermo_vertical(c, &x, stop);
    if (rc == 1) return 1;
    const std::string keep = c->err;
    if (rc == 0) {                            // (no merge after a stop)
        with_ncat(v.ncat, [&](auto NC) {
            with_bool(p != nullptr, [&](auto LVL) { rc = launch_blocks(c, k_therm1_merge<decltype(NC)::value, decltype(LVL)::value>, A); });
        });
        if (rc) return 1;
    }
    if (stage_out(c, arr)) return 1;
    if (rc) c->err = keep;
    return rc;
}

extern "C" int evpk_step_therm1(evpk_ctx *c, const evpk_therm1_args *a, int32_t stop[5]) {
    COLUMN_ENTRY(c, "evpk_step_therm1", stop, a && stop);
    return therm1_run(c, "evpk_step_therm1", a, nullptr, stop);
}

// step_therm1 under tr_pond_lvl: compute_ponds_lvl (source/ice_meltpond_lvl.F90:79-404) in the place of compute_ponds_cesm
extern "C" int evpk_step_therm1_lvl(evpk_ctx *c, const evpk_therm1_args *a, const evpk_pond_lvl_args *p, int32_t stop[5]) {
    COLUMN_ENTRY(c, "evpk_step_therm1_lvl", stop, a && p && stop);
    return therm1_run(c, "evpk_step_therm1_lvl", a, p, stop);
}

// ---- step_radiation (source/ice_step_mod.F90:1364-1524, ccsm3) with the albedo lines of coupling_prep, and prep_radiation (:33-145):
// one launch each (kernels in evpk_rad.hip) ----
extern "C" int evpk_step_radiation(evpk_ctx *c, const evpk_rad_args *a) {
    const char *who = "evpk_step_radiation";
    COLUMN_ENTRY(c, "evpk_step_radiation", NO_STOP, a);
    const evpk_itd_tracers &t = a->t;
    RadArgs A{};
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb, n3 = N * a->ncat;
    std::vector<HostArr> arr = {            // (every output is written on every cell: none is copied up)
        {a->aicen, n3, &A.aicen, false}, {a->vicen, n3, &A.vicen, false}, {a->vsnon, n3, &A.vsnon, false}, {a->trcrn, n3 * a->ntrcr_dim, &A.trcrn, false},
        {a->swvdr, N, &A.swvdr, false}, {a->swvdf, N, &A.swvdf, false}, {a->swidr, N, &A.swidr, false}, {a->swidf, N, &A.swidf, false},
        OptArr(a->ocn_albedo2D, N, &A.ocn_albedo2D, false),
        {a->alvdrn, n3, &A.alvdrn, true, false}, {a->alidrn, n3, &A.alidrn, true, false}, {a->alvdfn, n3, &A.alvdfn, true, false},
        {a->alidfn, n3, &A.alidfn, true, false}, {a->albicen, n3, &A.albicen, true, false}, {a->albsnon, n3, &A.albsnon, true, false},
        {a->fswsfcn, n3, &A.fswsfcn, true, false}, {a->fswintn, n3, &A.fswintn, true, false}, {a->fswthrun, n3, &A.fswthrun, true, false},
        {a->Sswabsn, n3 * t.nslyr, &A.Sswabsn, true, false}, {a->Iswabsn, n3 * t.nilyr, &A.Iswabsn, true, false},
        OptArr(a->fswpenln, n3 * (t.nilyr + 1), &A.fswpenln, true, false),
        {a->coszen, N, &A.coszen, true, false}, {a->alvdr, N, &A.alvdr, true, false}, {a->alidr, N, &A.alidr, true, false},
        {a->alvdf, N, &A.alvdf, true, false}, {a->alidf, N, &A.alidf, true, false}, {a->albice, N, &A.albice, true, false},
        {a->albsno, N, &A.albsno, true, false}, {a->scale_factor, N, &A.scale_factor, true, false}};
    if (a->shortwave_dEdd) FAIL(c, "%s: shortwave = 'dEdd' (run_dEdd) is not supported", who);
    if (flags_check(c, who, a->calc_Tsfc, a->heat_capacity)) return 1;
    if (any_missing(arr)) FAIL(c, "%s: a required argument is missing", who);
    if (layers_check(c, who, t.nilyr, t.nslyr, T1_MAXL) || ncat_check(c, who, a->ncat) ||
        Tsfc_check(c, who, a->ntrcr, a->ntrcr_dim, t.nt_Tsfc) || puny_check(c, who, a->puny))
        return 1;
    if (!c->nblocks) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    A.ncat = a->ncat; A.ntrcr_dim = a->ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb; A.nilyr = t.nilyr; A.nslyr = t.nslyr; A.nt_Tsfc = t.nt_Tsfc;
    A.constant_albedos = a->albedo_constant ? 1 : 0;
    A.puny = a->puny; A.albicev = a->albicev; A.albicei = a->albicei; A.albsnowv = a->albsnowv; A.albsnowi = a->albsnowi; A.ahmax = a->ahmax;
    A.snowpatch = a->snowpatch; A.albocn = a->albocn; A.awtvdr = a->awtvdr; A.awtidr = a->awtidr; A.awtvdf = a->awtvdf; A.awtidf = a->awtidf;
    if (stage_in(c, arr, true)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    int rc = 0;
    with_layers(a->ncat, t.nilyr, t.nslyr, [&](auto... S) { rc = launch_blocks(c, k_shortwave_ccsm3<decltype(S)::value...>, A); });
    return rc ? 1 : stage_out(c, arr);
}

extern "C" int evpk_prep_radiation(evpk_ctx *c, const evpk_prep_rad_args *a) {
    const char *who = "evpk_prep_radiation";
    COLUMN_ENTRY(c, "evpk_prep_radiation", NO_STOP, a);
    PrepRadArgs A{};
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb, n3 = N * a->ncat;
    std::vector<HostArr> arr = {            // (fswfac is copied up too: its ghost cells keep the caller's values)
        {a->aice, N, &A.aice, false}, {a->aicen, n3, &A.aicen, false}, {a->swvdr, N, &A.swvdr, false}, {a->swvdf, N, &A.swvdf, false},
        {a->swidr, N, &A.swidr, false}, {a->swidf, N, &A.swidf, false}, {a->alvdr_ai, N, &A.alvdr_ai, false}, {a->alvdf_ai, N, &A.alvdf_ai, false},
        {a->alidr_ai, N, &A.alidr_ai, false}, {a->alidf_ai, N, &A.alidf_ai, false},
        {a->scale_factor, N, &A.scale_factor, true}, {a->fswfac, N, &A.fswfac, true},
        {a->fswsfcn, n3, &A.fswsfcn, true}, {a->fswintn, n3, &A.fswintn, true}, {a->fswthrun, n3, &A.fswthrun, true},
        OptArr(a->fswpenln, n3 * (a->nilyr + 1), &A.fswpenln, true), {a->Sswabsn, n3 * a->nslyr, &A.Sswabsn, true},
        {a->Iswabsn, n3 * a->nilyr, &A.Iswabsn, true}};
    if (any_missing(arr)) FAIL(c, "%s: a required argument is missing", who);
    if (layers_check(c, who, a->nilyr, a->nslyr, T1_MAXL) || ncat_check(c, who, a->ncat) || puny_check(c, who, a->puny)) return 1;
    if (!c->nblocks) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    A.ncat = a->ncat; A.nxb = c->nxb; A.nyb = c->nyb; A.nilyr = a->nilyr; A.nslyr = a->nslyr; A.puny = a->puny;
    if (stage_in(c, arr, true)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    int rc = 0;
    with_layers(a->ncat, a->nilyr, a->nslyr, [&](auto... S) { rc = launch_blocks(c, k_prep_radiation<decltype(S)::value...>, A); });
    return rc ? 1 : stage_out(c, arr);
}

// ---- step_radiation on its Delta-Eddington branch (source/ice_step_mod.F90:1408-1451: run_dEdd, source/ice_shortwave.F90:1251-1577) with
// the albedo lines of coupling_prep: one launch (kernel in evpk_dedd.hip) ----
// p: the level-ice pond arguments of evpk_step_radiation_dedd_lvl, or null for evpk_step_radiation_dedd
static int dedd_run(evpk_ctx *c, const char *who, const evpk_dedd_args *a, const evpk_pond_lvl_args *p) {
    const evpk_itd_tracers &t = a->t;
    const bool cesm = a->tr_pond_cesm || t.tr_pond_cesm;
    DeddArgs A{};
    const size_t N = (size_t)c->nblocks * c->nyb * c->nxb, n3 = N * a->ncat;
    std::vector<HostArr> arr = {            // (every output is written on every cell: none is copied up; coszen is in / out)
        {a->aicen, n3, &A.aicen, false}, {a->vicen, n3, &A.vicen, false}, {a->vsnon, n3, &A.vsnon, false}, {a->trcrn, n3 * a->ntrcr_dim, &A.trcrn, false},
        {a->swvdr, N, &A.swvdr, false}, {a->swvdf, N, &A.swvdf, false}, {a->swidr, N, &A.swidr, false}, {a->swidf, N, &A.swidf, false},
        {a->coszen, N, &A.coszen, true},
        {a->alvdrn, n3, &A.alvdrn, true, false}, {a->alidrn, n3, &A.alidrn, true, false}, {a->alvdfn, n3, &A.alvdfn, true, false},
        {a->alidfn, n3, &A.alidfn, true, false}, {a->albicen, n3, &A.albicen, true, false}, {a->albsnon, n3, &A.albsnon, true, false},
        {a->albpndn, n3, &A.albpndn, true, false}, {a->apeffn, n3, &A.apeffn, true, false}, {a->snowfracn, n3, &A.snowfracn, true, false},
        {a->fswsfcn, n3, &A.fswsfcn, true, false}, {a->fswintn, n3, &A.fswintn, true, false}, {a->fswthrun, n3, &A.fswthrun, true, false},
        {a->Sswabsn, n3 * t.nslyr, &A.Sswabsn, true, false}, {a->Iswabsn, n3 * t.nilyr, &A.Iswabsn, true, false},
        OptArr(a->fswpenln, n3 * (t.nilyr + 1), &A.fswpenln, true, false),
        {a->alvdr, N, &A.alvdr, true, false}, {a->alidr, N, &A.alidr, true, false}, {a->alvdf, N, &A.alvdf, true, false},
        {a->alidf, N, &A.alidf, true, false}, {a->albice, N, &A.albice, true, false}, {a->albsno, N, &A.albsno, true, false},
        {a->albpnd, N, &A.albpnd, true, false}, {a->apeff_ai, N, &A.apeff_ai, true, false}, {a->scale_factor, N, &A.scale_factor, true, false},
        // (the pond arrays: dhsn is in / out on the listed cells; pond_lvl_check and the fsnow line below answer for them)
        OptArr(p ? p->dhsn : nullptr, n3, &A.dhsn, true), OptArr(p ? p->ffracn : nullptr, n3, &A.ffracn, false),
        OptArr(p ? p->fsnow : nullptr, N, &A.fsnow, false)};
    if (flags_check(c, who, a->calc_Tsfc, a->heat_capacity)) return 1;
    if (a->tr_aero) FAIL(c, "%s: aerosol tracers (tr_aero) are not supported", who);
    if (!p && (a->tr_pond_lvl || t.tr_pond_lvl)) FAIL(c, "%s: tr_pond_lvl (dhsn, ffracn) is not supported", who);
    if (p && !(a->tr_pond_lvl || t.tr_pond_lvl)) FAIL(c, "%s: tr_pond_lvl is not set", who);
    if (p && cesm) FAIL(c, "%s: tr_pond_cesm is set beside tr_pond_lvl", who);
    if (a->tr_pond_topo || t.tr_pond_topo) FAIL(c, "%s: tr_pond_topo is not supported", who);
    if (any_missing(arr)) FAIL(c, "%s: a required argument is missing", who);
    if (layers_check(c, who, t.nilyr, t.nslyr, DEDD_MAXL) || ncat_check(c, who, a->ncat) || Tsfc_check(c, who, a->ntrcr, a->ntrcr_dim, t.nt_Tsfc))
        return 1;
    if (cesm && (t.nt_apnd < 1 || t.nt_hpnd < 1 || t.nt_apnd > a->ntrcr || t.nt_hpnd > a->ntrcr))
        FAIL(c, "%s: tr_pond_cesm without nt_apnd / nt_hpnd in 1..ntrcr = %d", who, a->ntrcr);
    if (puny_check(c, who, a->puny)) return 1;
    if (!(a->dT_mlt > 0.0)) FAIL(c, "%s: dT_mlt = %g", who, a->dT_mlt);
    if (p) {
        if (pond_lvl_check(c, who, t, a->ntrcr, p)) return 1;
        if (!p->fsnow) FAIL(c, "%s: tr_pond_lvl needs fsnow", who);
        if (!(p->dt > 0.0)) FAIL(c, "%s: dt = %g", who, p->dt);
    }
    if (!c->nblocks) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    A.ncat = a->ncat; A.ntrcr_dim = a->ntrcr_dim; A.nxb = c->nxb; A.nyb = c->nyb; A.nilyr = t.nilyr; A.nslyr = t.nslyr; A.nt_Tsfc = t.nt_Tsfc;
    A.nt_apnd = t.nt_apnd; A.nt_hpnd = t.nt_hpnd; A.tr_pond_cesm = cesm ? 1 : 0;
    A.puny = a->puny; A.rhos = c->p.rhos; A.R_snw = a->R_snw; A.dT_mlt = a->dT_mlt; A.rsnw_mlt = a->rsnw_mlt; A.kalg = a->kalg; A.hs0 = a->hs0;
    A.pndaspect = a->pndaspect; A.awtvdr = a->awtvdr; A.awtidr = a->awtidr; A.awtvdf = a->awtvdf; A.awtidf = a->awtidf;
    dedd_iops(a->R_ice, a->R_pnd, A.iop);
    if (p) { A.nt_alvl = t.nt_alvl; A.nt_ipnd = p->nt_ipnd; A.linitonly = p->linitonly ? 1 : 0; A.hs1 = p->hs1; A.dt = p->dt; }
    if (stage_in(c, arr, true)) return 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (staged caller arrays are pageable)
    int rc = 0;
    with_layers(a->ncat, t.nilyr, t.nslyr, [&](auto... S) {
        with_bool(p != nullptr, [&](auto LVL) { rc = launch_blocks(c, k_shortwave_dedd<decltype(S)::value..., decltype(LVL)::value>, A); });
    });
    return rc ? 1 : stage_out(c, arr);
}

extern "C" int evpk_step_radiation_dedd(evpk_ctx *c, const evpk_dedd_args *a) {
    COLUMN_ENTRY(c, "evpk_step_radiation_dedd", NO_STOP, a);
    return dedd_run(c, "evpk_step_radiation_dedd", a, nullptr);
}

// step_radiation (dEdd) under tr_pond_lvl: the level-ice block of run_dEdd (source/ice_shortwave.F90:1450-1514) sets the ponds
extern "C" int evpk_step_radiation_dedd_lvl(evpk_ctx *c, const evpk_dedd_args *a, const evpk_pond_lvl_args *p) {
    COLUMN_ENTRY(c, "evpk_step_radiation_dedd_lvl", NO_STOP, a && p);
    return dedd_run(c, "evpk_step_radiation_dedd_lvl", a, p);
}

// the tables of evpk_dedd_tables.h by name (no context, no device): out[0 .. n), n the table's length; 1 for an unknown name or another n
extern "C" int evpk_dedd_table(const char *name, double *out, int32_t n) {
    using namespace dedd;
    if (!name || !out) return 1;
    struct Tab { const char *name; const double *p; int n; };
    const Tab tabs[] = {{"rsnw_tab", rsnw_tab, NMBRAD}, {"Qs_tab", &Qs_tab[0][0], NSPINT * NMBRAD}, {"ws_tab", &ws_tab[0][0], NSPINT * NMBRAD},
                        {"gs_tab", &gs_tab[0][0], NSPINT * NMBRAD},
                        {"ki_ssl_mn", ki_ssl_mn, NSPINT}, {"wi_ssl_mn", wi_ssl_mn, NSPINT}, {"gi_ssl_mn", gi_ssl_mn, NSPINT},
                        {"ki_dl_mn", ki_dl_mn, NSPINT}, {"wi_dl_mn", wi_dl_mn, NSPINT}, {"gi_dl_mn", gi_dl_mn, NSPINT},
                        {"ki_int_mn", ki_int_mn, NSPINT}, {"wi_int_mn", wi_int_mn, NSPINT}, {"gi_int_mn", gi_int_mn, NSPINT},
                        {"ki_p_ssl_mn", ki_p_ssl_mn, NSPINT}, {"wi_p_ssl_mn", wi_p_ssl_mn, NSPINT}, {"gi_p_ssl_mn", gi_p_ssl_mn, NSPINT},
                        {"ki_p_int_mn", ki_p_int_mn, NSPINT}, {"wi_p_int_mn", wi_p_int_mn, NSPINT}, {"gi_p_int_mn", gi_p_int_mn, NSPINT},
                        {"kw", kw, NSPINT}, {"ww", ww, NSPINT}, {"gw", gw, NSPINT}, {"gauspt", gauspt, NGMAX}, {"gauswt", gauswt, NGMAX},
                        {"scalars", scalars, NSCALARS}};
    for (const Tab &t : tabs)
        if (!strcmp(name, t.name)) {
            if (n != t.n) return 1;
            for (int q = 0; q < n; q++) out[q] = t.p[q];
            return 0;
        }
    return 1;
}
