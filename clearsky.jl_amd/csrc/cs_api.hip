// cs_api.hip -- host side of the C ABI declared in include/clearsky_hip.h (context, uploads, launches).
// Reference interfaces replaced are cited in the header; orchestration follows fluxes.jl:238-279 / :357-383.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/clearsky_hip.h"
#include "../../include/clearsky_hip_dev.h"
#include "cs_kernels.h"
#include "cs_par.h"

using namespace csdev;

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

thread_local int g_nlaunch = 0;   // kernel launches since the last reset (cs_column_run reports its count)
#define CS_LAUNCH(...) do { g_nlaunch++; hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// the three forms of the piece-table build (cs_kernels.h: sepzones_body, edgezones_body), by the values CS_WORK_TABLES documents
enum { TABLES_NONE = 0, TABLES_MERGED = 1, TABLES_LANES16 = 2, TABLES_ONE_THREAD = 3 };   // no matrix-core kernels; blocks of k_gas_setup_mx; k_mxzones16; k_mxzones
// How one Voigt / Lorentz launch group is run: everything that follows from sizes, settings and which buffers exist (voigt_plan, the one
// place that holds the rules).  line_sum_voigt launches by it, a column keeps the plan of its last run and cs_column_work counts from it.
// What depends on the state of the step -- the side streams, who clears the near-line plane, the fused apply -- is not in here.
struct VoigtPlan {
    bool lor;                   // the Lorentz body and the Lorentz series of the matrix-core pieces (no near-line tiers, no sub-tile cores, no 8-term tier)
    int nt64, ngrp;             // 64-point tiles; groups of 16 states
    int q0, ishift;             // first interval in use; tile -> interval of the smallest size (both 0 without interpolated wings)
    int near_prio;              // wave priority of k_voigt_sub / k_voigt_near (0, 3)
    bool use_sep, use_edge;     // node sums (k_cheb_nodes_mx) / window ends (k_voigt_edge_mx) on the matrix cores
    bool core;                  // ... and the window cores on sub-tiles (k_voigt_sub)
    int tables;                 // which kernel builds the piece tables (TABLES_*), as cs_column_work reports it
    bool nsplit4;               // k_cheb_nodes with four waves per (interval, state)
    int nsplit;                 // k_cheb_nodes_mx: intervals (from q0 on) the four waves of a block share ...
    unsigned nblk_mx;           // ... and its blocks
    bool far_R;                 // ... its far pieces on their level's nfar nodes (re-interpolation matrices in use), else on all 64
    bool far64_shared;          // ... on all 64 because every item is shared (CS_TUNE_FAR64_SHARED), not for want of the matrices
    int nfar[CS_MAX_LEVEL];
    int far_split;              // waves per tile of k_voigt_far
    bool edge_big;              // k_voigt_edge_mx<1>: one wave per (tile, group); else <4>
    int edge_phases;            // ... cuts a cut-off edge by the sub-tiles its lines reach (<1> only)
    bool tnodes;                // ... and sums the lines inside every point's cut-off on the 16 tile nodes
    int nrep;                   // near-line kernels: how many consecutive tiles a wave takes in turn
    bool near_both;             // ... both tiers in one launch
    int sub_lean;               // k_voigt_sub's range-only pass (CS_TUNE_SUB_LEAN)
    unsigned nb_zones, nb_iz, nb_sep, nb_edge;   // blocks of the zone, interval-zone and piece-table parts of the setup launches
};

// the flux kernel instances (NS: the column's stream count): k_rt<NS, true>; k_rt<NS, false>; k_rt_streams<NS>; k_flux_scan<NS, 5>; k_flux_scan<NS, 0>; k_flux_chunk3<NS>; k_flux_chunk<NS>
enum FluxKern { FK_RT_UD, FK_RT, FK_RT_STREAMS, FK_SCAN5, FK_SCAN, FK_CHUNK3, FK_CHUNK };
// How the flux stage of a step is run: everything that follows from sizes, settings and what the column holds (flux_plan, the one place
// that holds the rules).  launch_flux launches by it, a column keeps the plan of its last run, and cs_column_info and cs_column_work read that.
// One plan, stored at setup and completed at run: cs_column_setup stores the k_rt part (form 0, and how long `partial` must be) under the
// settings of that moment; every run hands it back to flux_plan, which keeps that part and decides under the settings of the run whether a fused
// form takes its place.  A batch asks for the k_rt part of its B columns.  What depends on the state of the step -- side streams, cascade, `rad` -- is not in here.
struct FluxPlan {
    int form;                   // 0 = k_rt / k_rt_streams reading finished cross-sections from HBM, 3 = k_flux_scan (short grids), 2 = k_flux_chunk (long grids)
    FluxKern kern, rt_kern;     // the instance that runs; the one form 0 runs, fixed at setup (FK_RT_STREAMS: a short grid for sigma_impl, too)
    int nt64, tiles;            // 64-point tiles; k_rt: tiles per block
    int nblk, threads; size_t shmem;   // blocks (per column), threads, dynamic LDS
    bool band_sum; int nfreduce;       // the last blocks of the kernel to finish add the block partials (FluxFuse::ticket); else k_freduce adds nfreduce per column (0: not launched)
    bool need_tau;              // the kernel writes the layer optical depths whether the caller wants them or not
    size_t npartial, gpartial;  // rows of 2 np partials `partial` must hold, and the row where the group sums start
    int flags;                  // the CS_DF_* of the flux stage
};

// which forms a step dispatched (cs_column_work CS_WORK_FAR_SPLIT ..): the fields of its last Voigt group, the flags (CS_DF_*) of the whole step
struct Dispatch { int far_split, tables, near_prio, streams, nodes_split, flags; };
// What the step being enqueued did, kept by the caller that enqueues it (run_impl, cs_column_batch) and reached by the launchers through
// GasPass::log (NULL: nobody asks)
struct PhPlan;
struct StepLog {
    Dispatch disp = {};
    int near_launches = 0;      // near-line launches, all groups
    int line_kernel = 0;        // what summed the per-point far lines of the last group: 0 = k_voigt_far, 1 = k_linesum<shape>, 2 = k_phco2
    // a Voigt group as planned; streams: 1 node sums, 2 near-line kernels on their side streams
    void voigt_group(const VoigtPlan &pl, int streams, bool near_memset)
    {
        disp.far_split = pl.far_split; disp.tables = pl.tables; disp.near_prio = pl.near_prio; disp.streams = streams;
        disp.nodes_split = pl.nsplit4 ? 1 : 0;
        disp.flags |= (pl.tnodes ? CS_DF_TNODES : 0) | (pl.far64_shared ? CS_DF_FAR64_SHARED : 0) | (near_memset ? CS_DF_NEAR_MEMSET : 0);
        if (!pl.lor) near_launches += pl.near_both ? 1 : 2;
        line_kernel = 0;
    }
    void phco2_group(const PhPlan &pl);   // a PHCO2 group as planned (defined below PhPlan)
};

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(CS_EHIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// owns one device allocation; move-only, so that `x = T()` frees what x held and containers of structs with DevBuf members can
// grow without double frees
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    hipError_t reserve(size_t n)
    {
        if (n <= bytes && p) return hipSuccess;
        release();
        if (n == 0) n = 8;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

template <class T> int upload(DevBuf &b, const T *h, size_t n, hipStream_t s)
{
    HIPCHK(b.reserve(n * sizeof(T)));
    if (n) HIPCHK(hipMemcpyAsync(b.p, h, n * sizeof(T), hipMemcpyHostToDevice, s));
    return CS_OK;
}

struct GasTable {
    bool present = false;
    uint64_t generation = 0;   // bumped by every cs_gas_upload into the slot (a resident column's windows belong to one generation)
    int64_t L = 0;
    int niso = 0;
    double mu_min = 0.0, mu_max = 0.0, ga_max = 0.0, gs_max = 0.0, na_min = 0.0, na_max = 0.0;
    // host mirror of the table (58 B per line): what a column merges when several of its gases share one launch set
    std::vector<double> h_nu, h_S, h_ga, h_gs, h_Epp, h_na, h_mu, h_cheb;
    std::vector<int16_t> h_iso;
    std::vector<int32_t> h_ncheb;
    std::vector<uint8_t> h_gid;                          // merged tables only: member index of each line
    std::vector<std::pair<int, uint64_t>> members;       // merged tables only: (slot, generation) of each member, in member order
    std::vector<double> h_da;                            // air pressure shifts delta_a [cm^-1/atm] (cs_gas_upload_par keeps them; empty: none)
    double da_max = 0.0;                                 // max |delta_a| over the table
    DevBuf nu, S, ga, gs, Epp, na, mu, iso, ncheb, cheb, sref, gid;
    mutable DevBuf da;                                   // h_da on the device, uploaded at the first CS_SHAPE_PSHIFT use (ensure_shifts)
    GasDev dev() const
    {
        GasDev g;
        g.L = L;
        g.nu = nu.as<double>(); g.S = S.as<double>(); g.ga = ga.as<double>(); g.gs = gs.as<double>();
        g.Epp = Epp.as<double>(); g.na = na.as<double>(); g.mu = mu.as<double>();
        g.iso = iso.as<int16_t>(); g.ncheb = ncheb.as<int32_t>(); g.cheb = cheb.as<double>();
        g.sref = sref.as<double>();
        g.gid = h_gid.empty() ? nullptr : gid.as<uint8_t>();
        g.da = da.as<double>();
        return g;
    }
};

struct TableDev {
    bool present = false;
    uint64_t generation = 0;   // bumped whenever the slot is (re)filled (cs_bake, cs_table_upload) or cleared: a resident column's weights
                               // W [nT * nP][K] belong to one generation's (T, P) grid
    int64_t nnu = 0;
    int nT = 0, nP = 0;
    std::vector<double> T, lnP, nu;
    DevBuf Z;  // [nT*nP][nnu] ln sigma
};

// AcceleratedAbsorber (absorbers.jl:114-203): ln sigma on pressure knots, per wavenumber
struct AccelDev {
    bool present = false;
    uint64_t generation = 0;   // bumped whenever the KNOTS of the slot change (cs_accel_upload; cs_accel_store with other knots) or it is
                               // cleared: a resident column's knot cells belong to one generation (new VALUES on the same knots keep it)
    int64_t nnu = 0;
    int nk = 0;
    std::vector<double> lnP, nu;   // knots (ascending), wavenumbers
    DevBuf L;                      // [nk][nnu]
};

struct CiaBandHost {
    std::vector<double> nu, T;
    DevBuf dnu, dlnk;
};
struct CiaDev {
    bool present = false;
    uint64_t generation = 0;   // bumped whenever the slot's bands change (a resident column's per-grid tables belong to one generation)
    std::vector<CiaBandHost> bands;
    int filled = 0;
};

// interpolated far wings: interval levels of a nu grid (descending interval size; intervals of all levels form one list)
struct ChebGrid {
    int nlev = 0, nItot = 0;
    int itv[CS_MAX_LEVEL] = {}, nI[CS_MAX_LEVEL] = {}, ioff[CS_MAX_LEVEL] = {};
    double span[CS_MAX_LEVEL] = {};   // widest interval of the level (cheb_build; 0: not known)
    DevBuf nodes;               // [nItot][64]
    DevBuf Cm[CS_MAX_LEVEL];    // [nI][64][itv]
    DevBuf Rc[CS_MAX_LEVEL];    // level l >= 1: [nI][64][64], the parent's node values carried to the nodes of an interval (k_cheb_cascade)
    DevBuf tnodes, tC;          // per 64-point tile: 16 Chebyshev nodes [tiles][16] and the matrix that carries values at them to the tile's points
                                // [tiles][16][64] (k_voigt_edge_mx: the window-end lines inside the cut-off of every point of the tile)
    bool tile_nodes_ok = false; // 16 nodes carry such lines to rounding on this grid (far_node_count of their distance; cheb_build)
};
// per gas on that grid: windows per level, zones [K][nItot], node sums F [nItot][64][Kpad]
struct GasInterp { int nlev = 0, l0 = 0; int nfar[CS_MAX_LEVEL] = {}; DevBuf iwin[CS_MAX_LEVEL], iz, F, sep, edge; };   // nfar: nodes for a level's far pieces (far_node_count)   // levels l0 .. nlev-1 of the grid are in use; sep: SepZone [K/16][nItot]
                                                                                          // (matrix-core node sums), edge: EdgeZone [K/16][tiles] (matrix-core pieces of the per-point sum)

// the windows of one launch group on one grid (build_windows): everything that is decided from the TABLE positions of its lines
struct GroupWindows {
    int64_t g0 = 0, g1 = 0;   // the included lines (included_range)
    int64_t jlo = 0, jhi = 0; // the lines some window can reach: what the records are written for
    int64_t pa = 0, pb = 0;   // the included lines whose records exist (the pedestals of codes 4, 6 come off over them)
    int64_t mb = 0;           // codes 5, 6: the mirror lines are [pa, mb) (vvh_mirror_end); = pa for every other code, which never reads it
    int xtiles = 0;           // longest XCD stretch of the far kernel's tile order, in tiles (wave_windows)
    double ds = 0.0;          // CS_SHAPE_PSHIFT: the largest shift of the group at the pressures of its states (shift_width), which widens all of the above
    int ntile256 = 0, nwin = 0;
    DevBuf J0, J1, win;       // [ntile256], [ntile256] (tile_windows), [nwin] WaveWin: the 64-point tiles and the far kernel's block order (wave_windows)
};
// what a launch group needs per state, for N states (upload_group_states)
struct GroupStates {
    DevBuf conc, Pp;          // [nmem][N] concentration and partial pressure of every member (conc: groups of a column only)
    DevBuf gmax;              // [N] max Lorentz width over the members (gamma_bound; Voigt fast path)
    std::vector<double> h_T, h_gmax;   // host copies of T and gmax [N] (ph_wide_regions: which chi-regions these states let PHCO2 interpolate)
    DevBuf lrt, qref;         // state_tables(): [N], [N][niso]
};
// ... and a table, a CIA pair, the accelerated absorber's knots (one builder and one launcher each): the column's own records, a batch's, the context's
struct TabStates { DevBuf W, conc; };                    // table_states: weights [nT * nP][N] and concentrations [N]
struct CiaStates { DevBuf st, rho1, rho2, rhoa, Tr; };   // cia_states: CiaState [nband][N]; the pair's densities [amagat] and the air's [cm^-3],
                                                         // [N] each; Tr: CS_CIA_RADIATION only, the temperatures [N], where R(nu, T) is formed
struct AccelStates { DevBuf cell, x, xa, xb; };          // accel_states: knot interval and the three abscissae of the LinearInterpolator formula, [N] each

struct ColTab {
    int slot = 0;
    uint64_t generation = 0;   // of the table slot the weights were formed for
    TabStates st;              // at the K node states
};
struct ColAccel {
    int slot = -1;             // -1: none
    uint64_t generation = 0;   // of the accelerated-absorber slot the cells were formed for
    AccelStates st;            // at the K node pressures
};
// what a CIA pair fixes on the column's grid, whatever the states (cia_grid; kept while the column names the same slots and generations)
struct CiaGrid {
    DevBuf bands;             // CiaBand [nband]: the addresses and sizes of the slot's band tables
    DevBuf fac;               // k_cia_tab: [K] Lo^2 rho1 rho2 / rhoa
    DevBuf tab, toff;         // k_cia_tab: ln k of every band at the temperature of every node state, [toff[b] + k * nb + c]
    DevBuf tband, cell, fx;   // k_flux: per 64-point tile the bands that reach it [ntile][CS_CIA_ACT] (-1: none), and per (slot, wavenumber)
                              // the sample cell of that band (-1: outside it) and the position in the cell
    int nband = 0;
    int maxnb = 0;            // samples of the longest band (k_cia_tab's grid)
    int max_overlap = 0;      // bands of this object reaching one 64-point tile of the column's grid, at most (k_flux holds CS_CIA_ACT)
};
struct ColCia {
    int slot = 0, flags = 0;
    uint64_t generation = 0;  // of the CIA slot the per-grid part was built from
    CiaGrid grid;
    CiaStates st;             // at the K node states
};

// a gas of the column as the caller named it (conc is laid out [ngas, K] over these)
struct UserGas {
    int slot = 0, shape = 0;
    double cut = 25.0;
    uint64_t generation = 0;
    int64_t pairs_per_state = -1, lines_in_range = 0;
    int64_t pairs_all = -1;   // CS_SHAPE_PSHIFT: pairs over all node states (the shifted centres move with the pressure)
};
// a launch group: one gas, or all Voigt (Lorentz) gases of the column with the same cut-off merged into ONE sorted line table --
// sigma_total = sum_g C_g sigma_g (absorbers.jl:84-95) and a per-(state, line) record carries everything gas-specific (the
// member's concentration and partial pressure enter in k_gas_setup), so the kernels see one table: one launch set per column
// instead of one per gas, and windows as dense as the column's lines together
struct ColGas {
    std::vector<int> mem;     // indices into Column::ugas
    const GasTable *tab = nullptr;   // ctx->gas[slot], or a merged table ...
    std::shared_ptr<const GasTable> hold;   // ... which the column shares with the context's cache (an eviction there cannot free it)
    int shape = 0;
    double cut = 25.0;
    GroupWindows w;           // the group's windows on the column's grid, widened by its largest shift at the node pressures (build_windows)
    GroupStates st;           // what the group needs per node state (upload_group_states; cs_column_update_state)
    int ph_mask = -1;         // PHCO2: the regions those states keep out of the levels (ph_wide_regions; -1 before the first upload)
    DevBuf zones;             // [K][ntile64] Zone
    GasInterp itp;            // interpolated far wings (nlev = 0: off)
    bool ped = false;         // shape code 4: shape is SH_VOIGT and launch_pedestal follows the line sum over [w.pa, w.pb)
    bool vvh = false;         // shape code 5: shape is SH_VOIGT, the records carry S / R(nul, T) and launch_vvh follows the line sum
                              // (shape code 6: ped and vvh, and launch_vvh_ped follows it instead of both)
    bool pshift = false;      // CS_SHAPE_PSHIFT, or shape code 7: records centred at nul + delta_a P / P0, summed by k_linesum<shape> over windows widened by w.ds
    // Voigt / Lorentz groups: how the column's own cross-section stage last ran the group (sigma_impl; a batch's chunked passes run on
    // buffers of their own and leave it alone).  planned: it has, since setup -- the group's windows and zones are written, and
    // cs_column_work counts them by this plan
    VoigtPlan plan;
    bool planned = false;
};

struct Column {
    double *F_dst = nullptr;   // cs_column_set_flux_dst: caller-owned device memory the band fluxes [2 np] are written to (NULL: the column's own F)
    double *flux_out() { return F_dst ? F_dst : F.as<double>(); }
    bool ready = false;
    int64_t nnu = 0;
    int np = 0, nl = 0, nlob = 0, K = 0, nstream = 0, ngas = 0, ntile = 0;
    FluxPlan flux = {}, flux_last = {};   // the setup-time part of the flux plan (flux_plan); the plan the last cs_column_run ran by
    bool has_extra = false, has_S = false, has_alb = false;
    int want_tau = CS_TAU_NONE;   // what cs_column_fetch's tau is (CS_TAU_*): nothing, the layer depths [nl][nnu] (tau), or k_depth's product (depth): D [nnu], tile sums [np][m_ntile()]
    bool depth_mode() const { return want_tau == CS_TAU_TOTAL || want_tau == CS_TAU_TILES; }
    int want_M = CS_M_NONE;    // what Mup / Mdn hold (CS_M_*): nothing, the planes [np][nnu], the boundary levels [2][nnu], tile sums [np][m_ntile()]
    int64_t m_ntile() const { return (nnu + 63) / 64; }
    // rows and row length of Mup / Mdn in the column's mode (kernel layout: level-major)
    int m_rows() const { return want_M == CS_M_EDGES ? 2 : np; }
    int64_t m_cols() const { return want_M == CS_M_TILES ? m_ntile() : nnu; }
    bool default_wts = false;  // trapezoid weights of the column's own grid (not a shard of a larger one)
    int64_t g_nnu = 0, g_start = 0;      // set by cs_fluxes_discretized_multi: this column is points [g_start, g_start + nnu) of a grid of
    double g_left = 0.0, g_right = 0.0;  // g_nnu points, with these neighbours left and right (what its trapezoid weights depend on)
    int interp = 0;            // the context's interpolation settings at setup time (packed)
    double g = 0, sigma_gray = 0, theta_s = 0;
    RtParams rt;
    std::vector<double> h_P, h_Pk, h_xs, h_nu;
    std::vector<UserGas> ugas;   // the caller's gases (ngas of them)
    std::vector<ColGas> gas;     // launch groups
    size_t maxL = 0;             // ... their longest table, whether one of them takes pedestals off (codes 4, 6), whether one is PHCO2 (setup)
    bool any_ped = false, has_phco2 = false;
    int merge = 1;               // the context's cs_set_merge at setup time
    uint64_t grid_id = 0;        // names this setup's nu grid (what the PHCO2 path keeps per grid: PhScratch)
    int launches = 0;            // kernel launches of the last cs_column_run
    bool near_live = false;      // the last cs_column_run left its near-line pairs in sigma2 (k_rt read both planes): cs_column_sigma_fetch folds them in
    hipStream_t last_stream = nullptr;   // the stream that run was enqueued on (cs_column_fetch waits for it, not for the whole device)
    // CS_TUNE_GRAPH: the step as ONE hipGraph launch (captured on the second run after a change, replayed from the third on):
    // kernel arguments are device addresses that stay put between cs_column_update_state calls, so only what changes launch
    // geometry or pointers (setup, tables, CIA pairs, accelerated absorber, spectra switched on or off) drops the graph -- and, for a
    // PHCO2 group, new states that change which chi-regions its levels carry (ph_wide_regions: cs_column_update_state compares), or any
    // rebuild of the context's PHCO2 levels since the capture (another grid, cut-off or region mask: graph_ph_builds)
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    int runs_since_change = 0;
    bool graph_near_live = false, graph_sigma_partial = false;   // what the captured run left in near_live / sigma_partial / launches / log_last: a
    int graph_launches = 0;                                      // replay leaves the same (cs_column_batch writes its own dispatch into log_last)
    uint64_t graph_ph_builds = 0;   // PhScratch::builds when the step was captured
    std::vector<ColTab> tab;
    std::vector<ColCia> cia;
    ColAccel accel;
    std::vector<double> h_Tk;
    DevBuf nu, wts, P, Pk, Tk, muk, Tlev, extra, S_toa, albedo;
    DevBuf hot, cold, sigma, sigma2, tau, depth, Mup, Mdn, partial, F, stage, ranges;   // sigma2: the near-line plane (k_voigt_near on a side stream)
    DevBuf ped;                // launch_pedestal's workspace for K states (columns with a code-4 group)
    DevBuf vvh;                // the line sum of a code-5 group that is not the column's first, before launch_vvh (K x nnu)
    DevBuf hot32;              // fp32 line records of mixed precision for K states (sigma_impl sizes them): the column's own, as hot and cold are --
                               // a captured step names them, so no other entry point may move them (batches and shape calls bring their own)
    DevBuf fluxdbg;            // k_flux_scan: phase time stamps of block 0 (CS_T15_SCAN_STAMPS; cs_column_work CS_WORK_FLUX_SCAN_NS ..)
    DevBuf ticket;             // k_flux: blocks finished (the last one adds the block partials up)
    StepLog log_last;            // of the last cs_column_run (cs_column_info out[6], out[7]); its disp also of the last cs_column_batch
    StepLog graph_log;           // log_last of the captured run
    bool sigma_partial = false;  // the last run finished the cross-sections on chip (k_flux): cs_column_sigma_fetch evaluates them again, in HBM
    ChebGrid cheb;             // interpolation levels of the nu grid (nlev = 0: off)
    DevBuf chebF;              // node sums F [nItot][64][Kpad], summed over the column's gases (k_cheb_nodes accumulates)
};

}  // namespace

static std::atomic<int> g_live_ctx{0};   // contexts alive in this process (the last cs_destroy stops the worker pool)
static void pool_stop();

static void drop_graph(Column &c)
{
    if (c.graph_exec) (void)hipGraphExecDestroy(c.graph_exec);
    if (c.graph) (void)hipGraphDestroy(c.graph);
    c.graph_exec = nullptr;
    c.graph = nullptr;
    c.runs_since_change = 0;
}

// The lab switches of a context (cs_set_tuning, cs_set_matrix_cores; include/clearsky_hip_dev.h describes each), one named field per
// switch.  set_tuning() and set_matrix_cores() below decode the caller's integers into it and are the only code that knows a key number
// or a bit of a key; a Settings{} is what cs_create sets.  Multi-valued switches keep the caller's integer as given.
struct Settings {
    int matrix_nodes = 1;           // cs_set_matrix_cores & 3: far-wing node sums and window ends on v_mfma_f64 -- 0 never, 1 where the grid fills the chip, 2 always
    bool matrix_core = true;        // cs_set_matrix_cores | 4 clears it: the window core on sub-tiles (k_voigt_sub + the second mask of k_voigt_edge_mx)
    bool fuse_apply = false;        // CS_TUNE_FUSE_APPLY: k_voigt_edge_mx carries the interpolated wings to the grid where the column has one launch group
    bool small_mx = true;           // CS_TUNE_SMALL_MX: the matrix-core kernels on short grids too (their four-waves-per-item variants)
    int nodes_stream = 2;           // CS_TUNE_NODES_STREAM: node sums on a side stream -- 0 never, 1 on short grids, 2 always
    double margin = kChebMargin;    // CS_TUNE_MARGIN (per cent): distance of an interval's interpolated set, in half-widths
    bool graph = false;             // CS_TUNE_GRAPH: cs_column_run replays the step as one hipGraph
    bool rt_streams = true;         // CS_TUNE_RT_STREAMS: k_rt_streams on short grids
    int nsplit_levels = 1;          // CS_TUNE_NSPLIT_LEVELS: interval sizes (largest first) whose node sums four waves share in k_cheb_nodes_mx
    int near_stream = 1;            // CS_TUNE_NEAR_STREAM: near-line kernels on a second side stream -- 0 never, 1 where it pays, 2 always
    int mx_min_states = 7;          // CS_TUNE_MX_MIN_STATES: states of a group beyond their series radius for a line to join its matrix-core node piece
    bool ph_own_core = false;       // CS_TUNE_PH_OWN_CORE: the pairs within 3 cm^-1 in k_phco2's own core loop
    int ph_nodes = 0;               // CS_TUNE_PH_NODES: PHCO2 levels -- bit 0: 64 nodes on every interval, bit 1: the tiles as 64-point intervals too
    bool far64 = false;             // CS_TUNE_FAR64: the far pieces of the matrix-core node sums on all 64 nodes
    int cascade = 0;                // CS_TUNE_CASCADE: levels folded into the smallest -- 0 where it pays (cascade_pays), 1 always, 2 never
    int nodes_split = 0;            // CS_TUNE_NODES_SPLIT: k_cheb_nodes with four waves per (interval, state) -- 0 on short grids, 1 always, 2 never
    bool edge_full = false;         // CS_TUNE_EDGE_FULL: k_voigt_edge_mx multiplies all four sub-tiles for every line of a cut-off edge
    int flux_form = 0;              // CS_TUNE_FLUX & CS_T15_FORM_MASK: cross-sections finished in the flux kernel -- 0 where it pays, 1 never, 2 always
    bool freduce_always = false;    // CS_T15_FREDUCE: the block partials always added by k_freduce
    bool chunk4 = false;            // CS_T15_CHUNK4: k_flux_chunk with four waves per SIMD
    bool tables_one_thread = false; // CS_T15_TABLES_ONE_THREAD: k_mxzones instead of k_mxzones16
    bool multi_recut = false;       // CS_T15_MULTI_RECUT: cs_fluxes_discretized_multi re-cuts its partition also on shared devices
    bool scan_stamps = false;       // CS_T15_SCAN_STAMPS: phase time stamps of block 0 of k_flux_scan
    bool no_cascade_aside = false;  // CS_T15_NO_CASCADE_ASIDE: no folding of the levels on the node-sum side stream of short grids
    bool scan_mid = false;          // CS_T15_SCAN_MID: the scan form also on grids of 1024 .. 4096 tiles
    bool scan_recompute = false;    // CS_T15_SCAN_RECOMPUTE: k_flux_scan forms a chunk's transmissivities again instead of keeping them
    int near_prio = 0;              // CS_TUNE_NEAR_PRIO & CS_T16_PRIO_MASK: issue priority for k_voigt_sub / k_voigt_near -- 0 from 512 tiles on, 1 never, 2 always
    bool near_two_launches = false; // CS_T16_NEAR_TWO_LAUNCHES: k_voigt_near<0> + <1> also where k_voigt_near_both would do
    bool far64_shared = false;      // CS_TUNE_FAR64_SHARED: far pieces of an item the four waves of a block share on all 64 nodes
    int sub_lean = 0;               // CS_TUNE_SUB_LEAN: k_voigt_sub's range-only pass -- 0 where the piece tables predict no series pair, 1 never, 2 first in every wave
    bool near_memset = false;       // CS_TUNE_NEAR_MEMSET: the near-line plane cleared by a memset instead of written by k_voigt_sub
    int tables_merge = 0;           // CS_TUNE_TABLES_MERGE: the piece tables as blocks of k_gas_setup's launch -- 0 below 1024 tiles, 1 never, 2 always
    int far_split = 0;              // CS_TUNE_FAR_SPLIT: waves per tile of k_voigt_far (1, 2, 4; 0 = by grid size)
    bool edge_points = false;       // CS_TUNE_EDGE_POINTS: every window-end line of k_voigt_edge_mx at the points, none on the tile's 16 nodes
};
static void set_matrix_cores(Settings &st, int on)
{
    st.matrix_core = (on & 4) == 0;   // (tuning / tests: | 4 keeps the tile-wide near-zone pass everywhere)
    st.matrix_nodes = (on & 3) > 2 ? 2 : (on & 3);
}
static void set_tuning(Settings &st, int key, int v)
{
    switch (key) {
    case CS_TUNE_FUSE_APPLY: st.fuse_apply = v != 0; break;
    case CS_TUNE_SMALL_MX: st.small_mx = v != 0; break;
    case CS_TUNE_NODES_STREAM: st.nodes_stream = v; break;
    case CS_TUNE_MARGIN: st.margin = v > 0 ? 0.01 * v : kChebMargin; break;
    case CS_TUNE_GRAPH: st.graph = v != 0; break;
    case CS_TUNE_RT_STREAMS: st.rt_streams = v != 0; break;
    case CS_TUNE_NSPLIT_LEVELS: st.nsplit_levels = v > 0 ? v : 1; break;
    case CS_TUNE_NEAR_STREAM: st.near_stream = v; break;
    case CS_TUNE_MX_MIN_STATES: st.mx_min_states = v > 0 ? v : 7; break;
    case CS_TUNE_PH_OWN_CORE: st.ph_own_core = v != 0; break;
    case CS_TUNE_PH_NODES: st.ph_nodes = v; break;
    case CS_TUNE_FAR64: st.far64 = v != 0; break;
    case CS_TUNE_CASCADE: st.cascade = v; break;
    case CS_TUNE_NODES_SPLIT: st.nodes_split = v; break;
    case CS_TUNE_EDGE_FULL: st.edge_full = v != 0; break;
    case CS_TUNE_FLUX:
        st.flux_form = v & CS_T15_FORM_MASK;
        st.freduce_always = (v & CS_T15_FREDUCE) != 0;
        st.chunk4 = (v & CS_T15_CHUNK4) != 0;
        st.tables_one_thread = (v & CS_T15_TABLES_ONE_THREAD) != 0;
        st.multi_recut = (v & CS_T15_MULTI_RECUT) != 0;
        st.scan_stamps = (v & CS_T15_SCAN_STAMPS) != 0;
        st.no_cascade_aside = (v & CS_T15_NO_CASCADE_ASIDE) != 0;
        st.scan_mid = (v & CS_T15_SCAN_MID) != 0;
        st.scan_recompute = (v & CS_T15_SCAN_RECOMPUTE) != 0;
        break;
    case CS_TUNE_NEAR_PRIO:
        st.near_prio = v & CS_T16_PRIO_MASK;
        st.near_two_launches = (v & CS_T16_NEAR_TWO_LAUNCHES) != 0;
        break;
    case CS_TUNE_FAR64_SHARED: st.far64_shared = v != 0; break;
    case CS_TUNE_SUB_LEAN: st.sub_lean = v; break;
    case CS_TUNE_NEAR_MEMSET: st.near_memset = v != 0; break;
    case CS_TUNE_TABLES_MERGE: st.tables_merge = v; break;
    case CS_TUNE_FAR_SPLIT: st.far_split = v; break;
    case CS_TUNE_EDGE_POINTS: st.edge_points = v != 0; break;
    default: break;   // (key 20: accepted, unused)
    }
}
// The settings a gas pass runs under (GasPass::set): the context's, or these defaults.  Today, as the call sites grew (DESIGN.md keeps the
// question open whether the last two should follow the context):
//   sigma_impl (the step of the resident column)       every group under the context's settings;
//   gas_states (cs_shape_batch, cs_shape_points,       under the context's where the call builds an interpolation view (cs_set_interp on and a
//     cs_bake) and cs_column_batch                      shape of the Voigt family | a group with interpolation levels), else under the defaults;
//   the inner Voigt pass of PHCO2 (line_sum_phco2)     always under the defaults.
// What a PHCO2 group itself reads of the context does not go through GasPass::set: the six inputs of PhRules (ph_rules) reach every PHCO2
// pass, from every entry point, with the grid (ph_set_grid).
static const Settings kDefaultSettings;

namespace {
// ---- the PHCO2 fast path (k_phco2) on the host: what it knows of a grid (PhGrid), what the context says about it (PhRules), the interpolation
// levels that follow from both (PhLevelSet, ph_levels), what built levels were built for (PhKey), and the context's workspace (PhScratch).
// How one group is run: PhPlan, below.

// the grid of a call: a function of (nu, nnu, id) and nothing else (ph_grid)
struct PhGrid {
    uint64_t id = 0;                               // names the grid: a column's setup, or one gas_states call (0: none)
    int64_t nnu = 0;
    double nu_lo = 0.0, nu_hi = 0.0, nu_c = 0.0;   // first and last point, and their mean: chi is factorised about nu_c
    double max_span = 0.0;                         // widest 64-point tile
    double lev_span[8] = {};                       // widest interval of 8192 >> i points
};
static PhGrid ph_grid(const double *nu, int64_t nnu, uint64_t id)
{
    PhGrid g;
    g.id = id; g.nnu = nnu;
    g.nu_lo = nu[0]; g.nu_hi = nu[nnu - 1];
    g.nu_c = 0.5 * (g.nu_lo + g.nu_hi);
    for (int64_t i0 = 0; i0 < nnu; i0 += 64) g.max_span = std::max(g.max_span, nu[std::min(i0 + 63, nnu - 1)] - nu[i0]);
    for (int i = 0; i < 8; i++) {
        const int64_t sz = 8192 >> i;
        double w = 0.0;
        for (int64_t i0 = 0; i0 < nnu; i0 += sz) w = std::max(w, nu[std::min(i0 + sz - 1, nnu - 1)] - nu[i0]);
        g.lev_span[i] = w;
    }
    return g;
}
// What the context says about PHCO2 (ph_rules); default-constructed: what cs_create sets.  PHCO2 passes follow the context for these six
// from every entry point -- the resident column, cs_column_batch, cs_shape_batch, cs_shape_points, cs_bake -- whatever GasPass::set is.
struct PhRules {
    bool itp_on = true;                               // cs_set_interp
    int itp_min = 128, itp_max = 2048;                // cs_set_interp_plan's size range
    double margin = kDefaultSettings.margin;          // Settings::margin
    int nodes = kDefaultSettings.ph_nodes;            // Settings::ph_nodes: 64 nodes for every interval (bit 0), tiles as 64-point intervals too (bit 1)
    bool own_core = kDefaultSettings.ph_own_core;     // Settings::ph_own_core
    bool operator==(const PhRules &o) const
    {
        return itp_on == o.itp_on && itp_min == o.itp_min && itp_max == o.itp_max && margin == o.margin && nodes == o.nodes && own_core == o.own_core;
    }
};
// interval sizes in use (descending) and the virtual levels on them (PhVLevels); nnodes = sum nI x nc, nslots = sum nI over the virtual levels
struct PhLevelSet {
    PhLevels lv; PhVLevels vl; PhFine fine;
    int nnodes = 0, nslots = 0;
};
// what a PhLevelSet follows from: the argument list of ph_levels, field by field (ph_key)
struct PhKey {
    uint64_t grid = 0;   // PhGrid::id (0: nothing built)
    int64_t nnu = 0;
    double cut = 0.0;
    int drop = 0;        // regions (bit r = region r + 1) the states of the launch keep out of the levels (ph_wide_regions)
    PhRules rules;
    bool operator==(const PhKey &o) const { return grid == o.grid && nnu == o.nnu && cut == o.cut && drop == o.drop && rules == o.rules; }
};
static PhKey ph_key(const PhGrid &g, const PhRules &rules, double cut, int drop)
{
    PhKey k;
    k.grid = g.id; k.nnu = g.nnu; k.cut = cut; k.drop = drop; k.rules = rules;
    return k;
}
// The context's PHCO2 workspace.  grid, rules: of the coming launch_gas calls, set together by the caller (ph_set_grid).  fac, win: per-(state,
// line) chi factors and per-tile region windows; win3, zones3: windows and zones of the Voigt pass over the pairs within 3 cm^-1; lev with
// nodes [sum nI x nc], Cm[v] [nI][nc][itv], piw, F: the interpolation levels (k_phco2_nodes) as built for `key` -- ph_prepare builds them
// again when a launch asks for another.  The scratch is one per context: two PHCO2 groups of one column whose keys differ (cut-offs,
// region masks) rebuild the levels for each other on every step.
struct PhScratch {
    DevBuf fac, win, piw, F, win3, zones3;
    PhGrid grid;
    PhRules rules;
    PhKey key;                 // what lev, nodes and Cm were laid out for: set only once every buffer of the levels is held, cleared when
    PhLevelSet lev;            // a build is refused, so that equal keys always mean built tables (phco2_plan then takes lev from here)
    DevBuf nodes, Cm[CS_MAX_ALEVEL];
    uint64_t builds = 0;       // how often ph_prepare has (re)built the levels or moved fac .. zones3: a captured step holds the layout of one build
    struct Dens { const void *tab; uint64_t gen, grid; bool ok; };
    std::vector<Dens> dens;    // check_near_density() per (table, generation, grid), a few kept (phco2_plan is the only reader)
};

// How one PHCO2 group of a pass is run, decided before its first launch (phco2_plan: the one place that holds the rules, as voigt_plan is
// for a Voigt group); ph_prepare reserves what the plan needs and takes back what it cannot have; line_sum_phco2 launches by it.  `key`
// and `lev` are ph_key and ph_levels of one argument list (lev: the scratch's own where it was built for that key).  The
// inner pass runs under kDefaultSettings, not under the context's: the open point of DESIGN.md, stated here and not decided.
struct PhPlan {
    bool fast = false;         // k_phco2; else k_linesum<SH_PHCO2> (line_sum_generic)
    int drop = 7;              // regions the states of the pass keep out of the levels (ph_wide_regions; 7 where the pass has no host states)
    bool levels = false;       // the far wings of the region-uniform lines on interpolation levels (k_phco2_nodes), `lev` of them
    bool build = false;        // ... whose tables this launch builds first (ph_prepare: the scratch held those of another key)
    bool clear_F = false;      // ... and whose node sums F it clears first (ph_prepare: F is new)
    bool inner = false;        // the pairs within 3 cm^-1 through the Voigt kernels; else k_phco2's own core loop
    int nt64 = 0;              // 64-point tiles
    unsigned nb_zones = 0;     // blocks of the zone part of k_gas_setup
    unsigned nb_tiles = 0, nb_itv = 0;   // blocks of k_phwin's tile part (once more for the inner pass's windows) and interval part
    PhKey key;
    PhLevelSet lev;
    void no_levels() { levels = build = clear_F = false; nb_itv = 0; }
};
inline void StepLog::phco2_group(const PhPlan &pl) { line_kernel = pl.fast ? 2 : 1; }
}  // namespace

// what cs_fluxes_discretized_multi keeps between calls (in its first context)
struct MultiPlan { int nctx = 0; std::vector<double> nu, wt; std::vector<uint64_t> gens; std::vector<int64_t> ranges; };

struct cs_ctx {
    PhScratch ph;
    MultiPlan mplan;
    int device = 0;
    bool counted = false;   // cs_create finished: the context counts in g_live_ctx
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;            // side stream: node sums beside the per-point kernels (Settings::nodes_stream)
    hipStream_t stream3 = nullptr;            // side stream: near-line kernels beside the matrix-core per-point kernel (Settings::near_stream)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fork3 = nullptr, ev_join3 = nullptr, ev_far3 = nullptr;
    GasTable gas[CS_MAX_GAS];
    TableDev tab[CS_MAX_TABLE];
    CiaDev cia[CS_MAX_CIA];
    AccelDev accel[CS_MAX_ACCEL];
    Column col;
    int mixed = 0;
    int interp = 1;   // far wings by Chebyshev interpolation over 128..2048-point intervals (k_cheb_nodes / k_cheb_apply)
    int itp_first = -1, itp_min = 128, itp_max = 2048;   // cs_set_interp_plan: first level per gas (-1 = by line density), size range
    int merge = 1;          // cs_set_merge: gases of a column with the same shape and cut-off share one merged line table
    Settings set;           // the lab switches: cs_set_tuning, cs_set_matrix_cores
    bool gfx950 = false;    // cs_create: the device reports gcnArchName gfx950 (the in-kernel band sum of k_flux_* is used only then)
    std::vector<std::shared_ptr<GasTable>> merged;   // merged tables (keyed by their members' (slot, generation)), least recently used first
    double far_s = 1e6;
    DevBuf reinterp;        // [64][32] then [64][16]: values at the 64 nodes of an interval from those at its 32 / 16 nodes (build_reinterp)
    DevBuf tmpA, tmpB, tmpC;   // cs_devfn_batch, cs_faddeeva_batch (A, B); the output of those and of cs_table_eval, cs_accel_eval (C) ...
    TabStates tmpTab; AccelStates tmpAccel;   // ... which evaluate at one state of their own: no step of the column names any of these
};
static PhRules ph_rules(const cs_ctx &ctx)
{
    PhRules r;
    r.itp_on = ctx.interp != 0; r.itp_min = ctx.itp_min; r.itp_max = ctx.itp_max;
    r.margin = ctx.set.margin; r.nodes = ctx.set.ph_nodes; r.own_core = ctx.set.ph_own_core;
    return r;
}
// the grid of the coming launch_gas calls (host copy `nu`), and the context's rules with it
static void ph_set_grid(cs_ctx *ctx, const double *nu, int64_t nnu, uint64_t grid_id)
{
    ctx->ph.grid = ph_grid(nu, nnu, grid_id);
    ctx->ph.rules = ph_rules(*ctx);
}

namespace {

// Gauss-Legendre / Gauss-Lobatto rules on [-1,1] (FastGaussQuadrature.gausslegendre / gausslobatto are the
// mathematically unique rules), ascending nodes.  Newton on P_n with the three-term recurrence.
void legendre(int n, double z, double &pn, double &pnm1)
{
    double p0 = 1.0, p1 = z;
    if (n == 0) { pn = 1.0; pnm1 = 0.0; return; }
    for (int j = 1; j < n; j++) {
        double p2 = ((2.0 * j + 1.0) * z * p1 - j * p0) / (j + 1.0);
        p0 = p1;
        p1 = p2;
    }
    pn = p1;
    pnm1 = p0;
}

void gauss_legendre(int n, double *x, double *w)
{
    for (int i = 0; i < n; i++) {
        double z = std::cos(M_PI * (i + 0.75) / (n + 0.5));
        double pn, pm, dp = 1.0;
        for (int it = 0; it < 64; it++) {
            legendre(n, z, pn, pm);
            dp = n * (z * pn - pm) / (z * z - 1.0);
            double dz = pn / dp;
            z -= dz;
            if (std::fabs(dz) < 1e-16) break;
        }
        legendre(n, z, pn, pm);
        dp = n * (z * pn - pm) / (z * z - 1.0);
        x[n - 1 - i] = z;
        w[n - 1 - i] = 2.0 / ((1.0 - z * z) * dp * dp);
    }
}

void gauss_lobatto(int n, double *x, double *w)
{
    const int N = n - 1;
    x[0] = -1.0;
    x[N] = 1.0;
    w[0] = w[N] = 2.0 / (N * (N + 1.0));
    for (int i = 1; i < N; i++) {
        double z = -std::cos(M_PI * i / N), pn, pm;
        for (int it = 0; it < 64; it++) {
            legendre(N, z, pn, pm);
            double d1 = N * (pm - z * pn) / (1.0 - z * z);
            double d2 = (2.0 * z * d1 - N * (N + 1.0) * pn) / (1.0 - z * z);
            double dz = d1 / d2;
            z -= dz;
            if (std::fabs(dz) < 1e-16) break;
        }
        legendre(N, z, pn, pm);
        x[i] = z;
        w[i] = 2.0 / (N * (N + 1.0) * pn * pn);
    }
}

// Lagrange basis of the interpolating polynomial on Chebyshev extrema x[0..n) (ascending), barycentric form:
// l_i(v) = (w_i/(v-x_i)) / sum_j (w_j/(v-x_j)),  w_i = (-1)^i * (1/2 at the two ends).  This is the unique polynomial
// BichebyshevInterpolator evaluates (gases.jl:80,85); only rounding can differ from the reference's algorithm.
void cheb_basis(const std::vector<double> &x, double v, std::vector<double> &l)
{
    const int n = (int)x.size();
    l.assign(n, 0.0);
    for (int i = 0; i < n; i++)
        if (v == x[i]) { l[i] = 1.0; return; }
    double den = 0.0;
    for (int i = 0; i < n; i++) {
        double w = ((i & 1) ? -1.0 : 1.0) * ((i == 0 || i == n - 1) ? 0.5 : 1.0);
        l[i] = w / (v - x[i]);
        den += l[i];
    }
    for (int i = 0; i < n; i++) l[i] /= den;
}

template <int SHAPE>
void launch_linesum(dim3 grid, hipStream_t s, const double *nu, int64_t nnu, int64_t L, const LineHot *hot,
                    const LineCold *cold, const int32_t *J0, const int32_t *J1, double cut, const double *Tk,
                    double base, const double *extra, double *sigma, int accumulate)
{
    CS_LAUNCH(k_linesum<SHAPE>, grid, dim3(256), 0, s, nu, nnu, L, hot, cold, J0, J1, cut, Tk, base, extra,
                       sigma, accumulate);
}

void launch_linesum_shape(int shape, dim3 grid, hipStream_t s, const double *nu, int64_t nnu, int64_t L,
                          const LineHot *hot, const LineCold *cold, const int32_t *J0, const int32_t *J1, double cut,
                          const double *Tk, double base, const double *extra, double *sigma, int accumulate)
{
    switch (shape) {
    case SH_LORENTZ: launch_linesum<SH_LORENTZ>(grid, s, nu, nnu, L, hot, cold, J0, J1, cut, Tk, base, extra, sigma, accumulate); break;
    case SH_DOPPLER: launch_linesum<SH_DOPPLER>(grid, s, nu, nnu, L, hot, cold, J0, J1, cut, Tk, base, extra, sigma, accumulate); break;
    case SH_PHCO2: launch_linesum<SH_PHCO2>(grid, s, nu, nnu, L, hot, cold, J0, J1, cut, Tk, base, extra, sigma, accumulate); break;
    default: launch_linesum<SH_VOIGT>(grid, s, nu, nnu, L, hot, cold, J0, J1, cut, Tk, base, extra, sigma, accumulate); break;
    }
}

// what every flux launch passes (host only; the kernels keep their argument lists, pointer by pointer)
struct FluxArgs {
    const RtParams *p;
    const double *nu, *wts;
    int64_t nnu;
    const double *sigma, *muk, *P, *Tlev, *S, *alb;   // S, alb: NULL without a stellar beam / an albedo
    double *tau, *Mup, *Mdn;                          // optional outputs
    double *partial;
    hipStream_t s;
};

// f(std::integral_constant<int, NS>) for the column's stream count: the one place that turns it into a template argument
template <class F>
void with_nstream(int ns, F &&f)
{
#define CS_NS(N) f(std::integral_constant<int, N>{}); break
    switch (ns) {
    case 1: CS_NS(1); case 2: CS_NS(2); case 3: CS_NS(3); case 4: CS_NS(4);
    case 5: CS_NS(5); case 6: CS_NS(6); case 7: CS_NS(7); case 8: CS_NS(8);
    case 9: CS_NS(9); case 10: CS_NS(10); case 11: CS_NS(11); case 12: CS_NS(12);
    case 13: CS_NS(13); case 14: CS_NS(14); case 15: CS_NS(15); case 16: CS_NS(16);
    }
#undef CS_NS
}

// a flux kernel with the arguments all of them begin with, then its own; more than 64 KB of dynamic LDS has to be asked for first
template <class Kern, class... Rest>
void launch_flux_kernel(Kern kern, dim3 grid, int threads, size_t shmem, const FluxArgs &a, Rest... rest)
{
    if (shmem > 65536) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    CS_LAUNCH(kern, grid, dim3(threads), shmem, a.s, *a.p, a.nu, a.wts, a.nnu, a.sigma, a.muk, a.P, a.Tlev, a.S, a.alb, a.tau, a.Mup, a.Mdn, a.partial,
              rest...);
}

// what flux_plan decides from, besides the settings: sizes; baked tables, launch groups, a CIA pair with more than CS_CIA_ACT bands over one tile; the device
struct FluxFacts { int64_t nnu; int np, nlob, K, nstream; bool tables, gases, cia_overlap, gfx950; int tau_mode; };   // (a step's choice of form alone reads the last five)

// The flux stage of a step (FluxPlan).  setup = NULL: the k_rt part for B columns, under these settings (cs_column_setup with B = 1;
// cs_column_batch); else the step of the resident column whose k_rt part is *setup, completed under these settings (run_impl).
// k_rt launch geometry: up/down split (two waves per 64-point tile) while the grid has fewer than ~4 waves per SIMD,
// tiles per block so that the grid still covers the chip
static FluxPlan flux_plan(const Settings &set, const FluxFacts &f, int B, const FluxPlan *setup)
{
    const int np = f.np, ns = f.nstream, nt64 = (int)((f.nnu + 63) / 64);
    const size_t lim = 160 * 1024 - 4096;   // dynamic LDS of one block
    if (!setup) {
        FluxPlan g = {};
        const int64_t nwave = (int64_t)nt64 * B; const bool ud = nwave < 4096;
        g.kern = ud ? FK_RT_UD : FK_RT; g.nt64 = nt64;
        g.tiles = ud ? (f.nnu >= 65536 ? 2 : 1) : (f.nnu >= 65536 ? 4 : 1);
        g.nblk = (int)((f.nnu + (int64_t)g.tiles * 64 - 1) / ((int64_t)g.tiles * 64));
        g.threads = g.tiles * 64 * (ud ? 2 : 1);
        g.shmem = ((size_t)2 * np * g.tiles + (ud ? (size_t)g.tiles * 64 : 0)) * sizeof(double);
        // short grids: the sweeps are latency chains -- one wave per (sweep, stream) of a tile instead of one per sweep (k_rt_streams): 1/8
        // of C3 (196 tiles) 0.061 -> 0.046 ms, C2 (157) 0.042 -> 0.033; from ~400 tiles on the two-wave form is as fast or faster (1/4 of
        // C3 0.082 vs 0.085, 1/2 0.087 vs 0.126: ten waves per tile stop fitting beside each other)
        const size_t sh2 = ((size_t)(2 * np - 1) * 64 + (size_t)4 * ns * 64 + (size_t)2 * np + 64) * sizeof(double);   // Planck + optical depths + exchange
        if (set.rt_streams && ud && g.tiles == 1 && nwave <= 400 && ns >= 2 && ns <= 8 && sh2 <= lim) {
            g.kern = FK_RT_STREAMS; g.flags = CS_DF_RT_STREAMS; g.threads = 2 * ns * 64; g.shmem = sh2;
        }
        g.rt_kern = g.kern; g.nfreduce = g.nblk;
        // a batch: the block partials of its B columns; the resident column: room for every form (one block per tile at most) + k_flux's group sums
        g.gpartial = (size_t)nt64; g.npartial = B > 1 ? (size_t)B * g.nblk : g.gpartial + 512 / CS_FLUX_GROUP;
        return g;
    }
    FluxPlan pl = *setup;
    if (set.flux_form == 1 || f.tables || !f.gases || f.cia_overlap) return pl;   // (baked tables are added between wings and CIA pairs: own pass)
    if (f.tau_mode == CS_TAU_TOTAL || f.tau_mode == CS_TAU_TILES) return pl;   // (k_depth reads the finished cross-sections from HBM: the fused forms never write them)
    const bool streams = pl.rt_kern == FK_RT_STREAMS, ud = pl.rt_kern != FK_RT;
    // the scan form: grids of up to 1024 tiles -- with a chunk's transmissivities in registers it beats the separate kernels on a half
    // (846 tiles: 1.10 -> 1.08 ms) and a quarter (407 tiles: 0.677 -> 0.610) of the bench column, not on the whole (1563 tiles: 1.94 ->
    // 1.99) -- and, under Settings::scan_mid, every grid in k_rt's two-waves-per-tile regime (A/B)
    // (Settings::flux_form = 2, `always`, keeps the chunked form on mid-size grids: tests)
    if (streams || (ud && ns >= 2 && ns <= 8 && nt64 >= 1 && ((nt64 <= 1024 && set.flux_form != 2) || set.scan_mid))) {
        // the sweeps as a scan over layer chunks: five layers per wave where 12 waves reach (their transmissivities stay in registers,
        // k_flux_scan<NS, 5>), whole waves per SIMD (4, 8 or 12: ten waves of six layers load two SIMDs with three waves and two with two)
        const int nw = std::min(12, std::max(4, 4 * ((np - 1 + 19) / 20))), per = (np - 1 + nw - 1) / nw;
        pl.shmem = ((size_t)f.K * 64 + (size_t)(2 * np - 1) * 64 + (size_t)2 * (ns + 1) * 64 + (size_t)2 * np) * sizeof(double);
        pl.form = 3; pl.nblk = nt64; pl.threads = nw * 64;
        // a chunk of up to 5 layers (60 layers over 12 waves) keeps its transmissivities in registers between the sweeps and passes
        // (seven streams and up: the 5 x NS values no longer fit beside the rest at three waves per SIMD)
        pl.kern = ns <= 6 && per <= 5 && !set.scan_recompute ? FK_SCAN5 : FK_SCAN;
    } else {
        // long grids: where k_rt runs one wave per tile for both sweeps (>= 4096 tiles) the chunked form saves the passes over the plane; in
        // between (the bench column at full size: 1563 tiles, two waves per tile) the separate kernels are as fast (profiles/r04_notes.md)
        if (set.flux_form != 2 && ud) return pl;
        const int nw = 4, R = 16 + f.nlob - 1;
        pl.shmem = ((size_t)2 * np * nw + (size_t)nw * R * 64) * sizeof(double);
        pl.form = 2; pl.nblk = (nt64 + nw - 1) / nw; pl.threads = nw * 64;
        pl.kern = set.chunk4 ? FK_CHUNK : FK_CHUNK3;
        // the chunked form always writes the layer optical depths (its upward sweep reads them back): into the caller's plane or scratch
        pl.need_tau = true;   // (forms 0 and 3 keep the optical depths in LDS unless the caller wants them)
    }
    if (pl.shmem > lim) return *setup;
    // up to 512 blocks the last ones to finish add the block partials (two stages of 16 and <= 32 terms); longer grids keep k_freduce
    pl.band_sum = pl.nblk <= 512 && !set.freduce_always && f.gfx950; pl.nfreduce = pl.band_sum ? 0 : pl.nblk;
    pl.flags = (pl.band_sum ? CS_DF_BAND_SUM : 0) | (pl.kern == FK_CHUNK ? CS_DF_CHUNK4 : 0);
    return pl;
}

// the flux kernel a plan names, for B columns.  The k_rt forms read finished cross-sections, sigma2 = the near-line plane (NULL: none);
// the fused forms (3 and 2) take *f.  rad: the column holds a CIA object flagged CS_CIA_RADIATION (kernels that can form R(nu, T_k);
// every other column runs the ones it always ran)
static int launch_flux(const FluxPlan &pl, int B, const FluxArgs &a, size_t sig_bstride, const double *sigma2, const FluxFuse *f = nullptr, bool rad = false)
{
    bool launched = false;
    auto go = [&](auto kern, const auto &... rest) { launch_flux_kernel(kern, dim3(pl.nblk, B), pl.threads, pl.shmem, a, rest...); launched = true; };
    if (pl.form == 0)
        with_nstream(a.p->nstream, [&](auto ns) {
            constexpr int NS = decltype(ns)::value;
            switch (pl.kern) {
            case FK_RT_STREAMS: if constexpr (NS >= 2 && NS <= 8) go(k_rt_streams<NS>, sig_bstride, sigma2); break;
            case FK_RT_UD: go(k_rt<NS, true>, sig_bstride, sigma2); break;
            case FK_RT: go(k_rt<NS, false>, sig_bstride, sigma2); break;
            default: break;
            }
        });
    else   // (a second pass over the stream counts: the instances keep their places in the code object)
        with_nstream(a.p->nstream, [&](auto ns) {
            constexpr int NS = decltype(ns)::value;
            auto fused = [&](auto radc) {
                constexpr bool RAD = decltype(radc)::value;
                switch (pl.kern) {
                case FK_SCAN5: if constexpr (NS >= 2 && NS <= 6) go(k_flux_scan<NS, 5, RAD>, *f); break;
                case FK_SCAN: if constexpr (NS >= 2 && NS <= 8) go(k_flux_scan<NS, 0, RAD>, *f); break;
                case FK_CHUNK3: go(k_flux_chunk3<NS, RAD>, *f, pl.nt64); break;
                case FK_CHUNK: go(k_flux_chunk<NS, RAD>, *f, pl.nt64); break;
                default: break;
                }
            };
            rad ? fused(std::true_type{}) : fused(std::false_type{});
        });
    return launched ? CS_OK : fail(CS_EINVAL, "internal: no flux kernel instance %d for %d streams", (int)pl.kern, a.p->nstream);
}

// includedlines(::Vector) line_shapes.jl:18-22 -> [g0, g1) ; strict = 0 keeps every line (scalar-nu method :12-16)
void included_range(const std::vector<double> &nul, double numin, double numax, double cut, bool strict, int64_t &g0,
                    int64_t &g1)
{
    const int64_t L = (int64_t)nul.size();
    g0 = 0;
    g1 = L;
    if (strict) {
        const double lo = numin - cut, hi = numax + cut;
        while (g0 < L && !(nul[g0] > lo)) g0++;
        while (g1 > g0 && !(nul[g1 - 1] < hi)) g1--;
    }
}

// per-tile union windows (a superset of every lane's |nu - nul| <= cut run; the kernel applies the exact test)
void tile_windows(const std::vector<double> &nul, int64_t g0, int64_t g1, const double *nu, int64_t nnu, double cut,
                  std::vector<int32_t> &J0, std::vector<int32_t> &J1)
{
    const int ntile = (int)((nnu + 255) / 256);
    J0.resize(ntile);
    J1.resize(ntile);
    auto b = nul.begin() + g0, e = nul.begin() + g1;
    for (int t = 0; t < ntile; t++) {
        const int64_t i0 = (int64_t)t * 256, i1 = std::min<int64_t>(nnu, i0 + 256) - 1;
        const double lo = nu[i0] - cut, hi = nu[i1] + cut;
        const double tol = 1e-9 * (std::fabs(hi) + cut + 1.0);
        J0[t] = (int32_t)(std::lower_bound(b, e, lo - tol) - nul.begin());
        J1[t] = (int32_t)(std::upper_bound(b, e, hi + tol) - nul.begin());
    }
}

// The far kernel hands k_voigt_near the near-line ranges of every (nu, node) as 20-bit offsets into the tile's near zone and
// 12-bit counts.  Bound both for any state (widest Doppler width: upper end of the grid, TMAX, lightest isotopologue) and
// refuse tables too dense for the fields -- 4096 lines within a few Doppler widths is ~1e5 lines per cm^-1, far beyond HITEMP.
int check_near_density(const GasTable &G, double nu_hi, double span, double cut, double ds = 0.0);
int check_near_density(const GasTable &G, const double *nu, int64_t nnu, double cut, double ds = 0.0)
{
    double span = 0.0;
    for (int64_t i0 = 0; i0 < nnu; i0 += 64) span = std::max(span, nu[std::min<int64_t>(i0 + 63, nnu - 1)] - nu[i0]);
    return check_near_density(G, nu[nnu - 1], span, cut, ds);
}
// span: widest 64-point tile of the grid; ds: largest line shift of a CS_SHAPE_PSHIFT group (its zones and ranges span 2 ds more)
int check_near_density(const GasTable &G, double nu_hi, double span, double cut, double ds)
{
    const double amax = ((nu_hi + cut) / kC) * std::sqrt(2.0 * kRgas * kTmax / G.mu_min);
    const double dA = 100.0 * amax / kSqLn2 * (1.0 + 1e-6), r0 = std::sqrt(kSerS) * amax / kSqLn2 * 1.01;
    const std::vector<double> &v = G.h_nu;
    auto max_in = [&](double width) {
        int64_t best = 0;
        size_t a = 0;
        for (size_t b = 0; b < v.size(); b++) {
            while (v[b] - v[a] > width) a++;
            best = std::max<int64_t>(best, (int64_t)(b - a + 1));
        }
        return best;
    };
    const int64_t nzone = max_in(span + 2.0 * dA + 2.0 * ds), npt = max_in(2.0 * r0 + 2.0 * ds);
    if (nzone >= (1 << kNearFirstBits) || npt >= (1 << kNearCountBits))
        return fail(CS_EINVAL, "line table too dense for the near-line hand-off: %lld lines within %.3g cm^-1, %lld within %.3g cm^-1",
                    (long long)nzone, span + 2.0 * dA, (long long)npt, 2.0 * r0);
    return CS_OK;
}

// Doppler profile exp(-(dnu/alpha)^2) (line_shapes.jl:160): beyond sqrt(750) widths it is an exact zero in fp64 (exp(-745.2) is
// the smallest denormal), so the windows of the Doppler line sum only need the lines within that reach of a tile -- a bound for
// every state: the widest line is the one at the upper end of the grid, at TMAX, of the lightest isotopologue (line_shapes.jl:144)
double window_reach(int shape, const GasTable &G, double numax, double cut)
{
    if (shape != SH_DOPPLER) return cut;
    const double amax = ((numax + cut) / kC) * std::sqrt(2.0 * kRgas * kTmax / G.mu_min);
    return std::min(cut, std::sqrt(750.0) * amax * (1.0 + 1e-6));
}

int64_t count_pairs(const std::vector<double> &nul, const double *nu, int64_t nnu, double cut)
{
    int64_t pairs = 0;
    for (int64_t i = 0; i < nnu; i++)
        pairs += (std::upper_bound(nul.begin(), nul.end(), nu[i] + cut) - std::lower_bound(nul.begin(), nul.end(), nu[i] - cut));
    return pairs;
}

// per-64-point windows of the Voigt fast path: [W0,W1) superset window, [E0,E1) lines inside every lane's cut-off
// For span == 64 (the tiles of k_voigt_far) three more entries follow the nt windows: the block order of that kernel (tile_block).
// xc[0..8] = tile indices (multiples of 4) of eight contiguous stretches of the spectrum, one per XCD, when the line table is
// dense enough for its records to matter in that kernel's HBM traffic (32 B x lines against 16 B x wavenumbers per state:
// contiguous from L >= nnu / 8); xc[0] = -1 = plain block order otherwise.  Returns the number of tiles per XCD (grid size).
// ds > 0 (CS_SHAPE_PSHIFT): every line sits within ds of its table position -- the tile is widened by ds on both sides, so that [W0,W1)
// holds every line that can reach it and [E0,E1) only lines inside every lane's cut-off wherever they are shifted to
int wave_windows(const std::vector<double> &nul, int64_t g0, int64_t g1, const double *nu, int64_t nnu, double cut,
                 std::vector<WaveWin> &win, int span = 64, double ds = 0.0)
{
    const int nt = (int)((nnu + span - 1) / span);
    win.resize(nt);
    auto b = nul.begin() + g0, e = nul.begin() + g1;
    for (int t = 0; t < nt; t++) {
        const int64_t i0 = (int64_t)t * span, i1 = std::min<int64_t>(nnu, i0 + span) - 1;
        const double vlo = nu[i0] - ds, vhi = nu[i1] + ds;
        const double tol = 1e-9 * (std::fabs(vhi) + cut + 1.0);
        WaveWin w;
        w.W0 = (int32_t)(std::lower_bound(b, e, vlo - cut - tol) - nul.begin());
        w.W1 = (int32_t)(std::upper_bound(b, e, vhi + cut + tol) - nul.begin());
        w.E0 = (int32_t)(std::lower_bound(b, e, vhi - cut + tol) - nul.begin());
        w.E1 = (int32_t)(std::upper_bound(b, e, vlo + cut - tol) - nul.begin());
        w.E0 = std::min(std::max(w.E0, w.W0), w.W1);
        w.E1 = std::min(std::max(w.E1, w.E0), w.W1);
        win[t] = w;
    }
    if (span != 64) return 0;
    int32_t xc[12] = {0};
    const int nt4 = (nt + 3) / 4 * 4;
    const int per = ((nt4 / 4 + 7) / 8) * 4;      // tiles per XCD, a multiple of 4
    const int64_t inrange = (std::upper_bound(b, e, nu[nnu - 1] + cut + ds) - std::lower_bound(b, e, nu[0] - cut - ds));
    for (int x = 0; x <= 8; x++) xc[x] = std::min(x * per, nt4);
    if (inrange * 8 < nnu) xc[0] = -1;
    win.resize(nt + 3);
    memcpy(&win[nt], xc, sizeof xc);
    return per;
}

// upper bound of gammalorentz (line_shapes.jl:255-257) over a gas's lines at every state
std::vector<double> gamma_bound(const GasTable &G, int K, const double *T, const double *P, const double *Pp)
{
    std::vector<double> g(K);
    for (int k = 0; k < K; k++) {
        const double r = kTref / T[k];
        const double f = std::max(std::pow(r, G.na_min), std::pow(r, G.na_max));
        g[k] = f * (std::fabs(G.ga_max * (P[k] - Pp[k])) + std::fabs(G.gs_max * Pp[k])) / kAtm * (1.0 + 1e-12);
    }
    return g;
}

// what k_gas_setup needs per state alone: ln(Tref/T) and Qref/Q(T) of every isotopologue of the table (line_shapes.jl:27-48)
void state_tables(const GasTable &G, int K, const double *T, std::vector<double> &lrt, std::vector<double> &qrefq)
{
    lrt.resize(K);
    qrefq.assign((size_t)K * G.niso, 0.0);
    for (int k = 0; k < K; k++) {
        lrt[k] = std::log(kTref / T[k]);
        for (int i = 0; i < G.niso; i++)
            if (G.h_ncheb[i] > 0) qrefq[(size_t)k * G.niso + i] = cheby_qrefq(T[k], G.h_ncheb[i], G.h_cheb.data() + (size_t)i * CS_CHEB_LD);
    }
}

// far wings by interpolation (k_cheb_nodes + k_cheb_apply), view handed to launch_gas; nlev = 0: off
struct Interp {
    int nlev = 0, nItot = 0, Kpad = 0, l0 = 0;
    int itv[CS_MAX_LEVEL], nI[CS_MAX_LEVEL], ioff[CS_MAX_LEVEL];
    const double *nodes = nullptr, *Cm[CS_MAX_LEVEL];
    const WaveWin *iwin[CS_MAX_LEVEL];
    IZone *iz = nullptr;
    double *F = nullptr;
    SepZone *sep = nullptr;   // NULL: every node sum on the vector unit
    EdgeZone *edge = nullptr; // NULL: all of the per-point sum on the vector unit
    int nfar[CS_MAX_LEVEL] = {};   // nodes for the far pieces of a level in k_cheb_nodes_mx (16, 32; 64 = as the near pieces)
    const double *Rc[CS_MAX_LEVEL] = {};   // ChebGrid::Rc
    const double *R = nullptr;     // the context's re-interpolation matrices (cs_ctx::reinterp); NULL: every piece on 64 nodes (CS_TUNE_FAR64)
    const double *tnodes = nullptr, *tC = nullptr;   // ChebGrid::tnodes, tC where the grid allows (tile_nodes_ok) and CS_TUNE_EDGE_POINTS = 0
};

// the buffers of a view that the context's settings select
static void interp_select(const cs_ctx *ctx, Interp &itp)
{
    if (!ctx->set.matrix_nodes) itp.sep = nullptr, itp.edge = nullptr;
    itp.R = ctx->set.far64 ? nullptr : ctx->reinterp.as<double>();
    if (ctx->set.edge_points) itp.tnodes = itp.tC = nullptr;
}

// interval sizes worth using on this grid: an interval of width W leaves lines over (2 cut - 2.3 W) to interpolate
int choose_levels(double nu_lo, double nu_hi, int64_t nnu, double cut, int *itv, int szmin = 128, int szmax = 2048)
{
    int n = 0;
    if (nnu < 128) return 0;
    const double dnu = (nu_hi - nu_lo) / (double)(nnu - 1);
    for (int sz = 8192; sz >= 128 && n < CS_MAX_LEVEL; sz >>= 1)
        if (sz <= szmax && sz >= szmin && 2.3 * sz * dnu <= 1.5 * cut && sz / 2 <= nnu &&
            sz * dnu > 1e-8 * std::fabs(nu_hi))   // (nodes 1e-3 of an interval apart must stay distinct doubles)
            itv[n++] = sz;
    return n;
}
int choose_levels(const double *nu, int64_t nnu, double cut, int *itv, int szmin = 128, int szmax = 2048)
{
    return nnu < 1 ? 0 : choose_levels(nu[0], nu[nnu - 1], nnu, cut, itv, szmin, szmax);
}

// the grid part: nodes [nItot][64] and interpolation matrices [nI][64][itv] per level
int cheb_build_range(ChebGrid &g, double nu_lo, double nu_hi, const double *dnu, int64_t nnu, double cut, int szmin, int szmax, hipStream_t s);
int far_node_count(double dist, double h);
int cheb_build(const cs_ctx *ctx, ChebGrid &g, const double *h_nu, const double *dnu, int64_t nnu, double cut, hipStream_t s)
{
    const int rc = cheb_build_range(g, h_nu[0], h_nu[nnu - 1], dnu, nnu, cut, ctx->itp_min, ctx->itp_max, s);
    for (int l = 0; l < g.nlev; l++) {
        g.span[l] = 0.0;
        for (int64_t i0 = 0; i0 < nnu; i0 += g.itv[l]) g.span[l] = std::max(g.span[l], h_nu[std::min<int64_t>(i0 + g.itv[l] - 1, nnu - 1)] - h_nu[i0]);
    }
    // the window-end lines inside the cut-off of every point of a tile are at least cut-off - (smallest interval) - (tile) from it:
    // 16 nodes of the tile carry their sum to rounding where far_node_count says so (23 cm^-1 from a 1.6 cm^-1 tile: by far)
    g.tile_nodes_ok = false;
    if (g.nlev > 0) {
        double tspan = 0.0;
        for (int64_t i0 = 0; i0 < nnu; i0 += 64) tspan = std::max(tspan, h_nu[std::min<int64_t>(i0 + 63, nnu - 1)] - h_nu[i0]);
        const double dist = cut - g.span[g.nlev - 1] - tspan;
        g.tile_nodes_ok = tspan > 0.0 && dist > 0.0 && far_node_count(dist, 0.5 * tspan) == 16;
    }
    return rc;
}
// nodes for a set of lines that stays `dist` away from intervals of half-width h: the interpolation error falls like rho^-(n-1),
// rho = x0 + sqrt(x0^2 - 1), x0 = 1 + dist / h; 1e-18 asked for (64 nodes at the margin of 0.3: rho = 2.1, 5e-21)
int far_node_count(double dist, double h)
{
    if (!(dist > 0.0) || !(h > 0.0)) return CS_NC;
    const double x0 = 1.0 + dist / h, lr = std::log10(x0 + std::sqrt(x0 * x0 - 1.0));
    return 15.0 * lr >= 18.0 ? 16 : (31.0 * lr >= 18.0 ? 32 : CS_NC);
}
int cheb_build_range(ChebGrid &g, double nu_lo, double nu_hi, const double *dnu, int64_t nnu, double cut, int szmin, int szmax, hipStream_t s)
{
    g.nlev = choose_levels(nu_lo, nu_hi, nnu, cut, g.itv, szmin, szmax);
    g.nItot = 0;
    for (int l = 0; l < g.nlev; l++) {
        g.nI[l] = (int)((nnu + g.itv[l] - 1) / g.itv[l]);
        g.ioff[l] = g.nItot;
        g.nItot += g.nI[l];
    }
    if (g.nlev == 0) return CS_OK;
    HIPCHK(g.nodes.reserve((size_t)g.nItot * CS_NC * sizeof(double)));
    for (int l = 0; l < g.nlev; l++) {
        HIPCHK(g.Cm[l].reserve((size_t)g.nI[l] * CS_NC * g.itv[l] * sizeof(double)));
        CS_LAUNCH(k_cheb_setup, dim3(g.nI[l]), dim3(256), 0, s, dnu, nnu, g.itv[l], g.nI[l], CS_NC,
                           g.nodes.as<double>() + (size_t)g.ioff[l] * CS_NC, g.Cm[l].as<double>());
        HIPCHK(hipGetLastError());
    }
    for (int l = 1; l < g.nlev; l++) {
        int pshift = 0;
        for (int r = g.itv[l - 1] / g.itv[l]; r > 1; r >>= 1) pshift++;
        HIPCHK(g.Rc[l].reserve((size_t)g.nI[l] * CS_NC * CS_NC * sizeof(double)));
        CS_LAUNCH(k_cascade_setup, dim3(g.nI[l]), dim3(256), 0, s, g.nodes.as<double>(), g.ioff[l - 1], g.ioff[l], pshift, g.Rc[l].as<double>());
        HIPCHK(hipGetLastError());
    }
    {   // the tiles as intervals of their own with 16 nodes (k_voigt_edge_mx's node path)
        const int nt64 = (int)((nnu + 63) / 64);
        HIPCHK(g.tnodes.reserve((size_t)nt64 * 16 * sizeof(double)));
        HIPCHK(g.tC.reserve((size_t)nt64 * 16 * 64 * sizeof(double)));
        CS_LAUNCH(k_cheb_setup, dim3(nt64), dim3(256), 0, s, dnu, nnu, 64, nt64, 16, g.tnodes.as<double>(), g.tC.as<double>());
        HIPCHK(hipGetLastError());
    }
    return CS_OK;
}

int cheb_kpad(int K) { return (K + CS_KPAD - 1) / CS_KPAD * CS_KPAD; }

// the gas part: per-level interval windows (uploaded) and zone workspace for K states; F workspace of the grid
// First level worth using for a gas with `lambda` lines per cm^-1 (work per (nu, state) in line evaluations): a level costs
// ~4.4 evaluations in k_cheb_apply whatever the table, and saves (lines of its set) x (1/r_next - 1/r), r = interval size / 64.
int choose_l0(const ChebGrid &g, const double *nu, int64_t nnu, double cut, double lambda)
{
    const double dnu = (nu[nnu - 1] - nu[0]) / (double)std::max<int64_t>(nnu - 1, 1);
    int best = g.nlev;
    double bestc = 1e300;
    for (int l0 = 0; l0 <= g.nlev; l0++) {
        double c = 0.0;
        if (l0 == g.nlev) {
            c = 1.05 * 2.0 * cut * lambda;   // every pair evaluated directly
        } else {
            const double Wtop = g.itv[l0] * dnu;
            c += std::max(2.0 * cut - 2.3 * Wtop, 0.0) * lambda * 64.0 / g.itv[l0];
            for (int l = l0 + 1; l < g.nlev; l++) c += 2.3 * (g.itv[l - 1] - g.itv[l]) * dnu * lambda * 64.0 / g.itv[l];
            c += (2.3 * g.itv[g.nlev - 1] + 64.0) * dnu * lambda * 1.4;   // left to the per-point kernels
            c += 4.4 * (g.nlev - l0);
        }
        if (c < bestc) { bestc = c; best = l0; }
    }
    return best;
}

int gas_interp_build(const cs_ctx *ctx, GasInterp &gi, ChebGrid &g, const std::vector<double> &nul, int64_t g0, int64_t g1,
                     const double *nu, int64_t nnu, double cut, int K, hipStream_t s, bool own_F = true, double ds = 0.0)
{
    int rc;
    gi.nlev = g.nlev;
    gi.l0 = 0;
    if (g.nlev == 0) return CS_OK;
    {
        const double span = nu[nnu - 1] - nu[0] + 2.0 * cut;
        const auto b = std::lower_bound(nul.begin() + g0, nul.begin() + g1, nu[0] - cut);
        const auto e = std::upper_bound(nul.begin() + g0, nul.begin() + g1, nu[nnu - 1] + cut);
        gi.l0 = choose_l0(g, nu, nnu, cut, (double)(e - b) / span);
        if (ctx->itp_first >= 0) gi.l0 = std::min(ctx->itp_first, g.nlev);
        if (gi.l0 >= g.nlev) { gi.nlev = 0; gi.l0 = 0; return CS_OK; }   // too few lines: every pair directly
    }
    // far pieces of a level (the lines beyond its parent's set): at least cut-off minus the parent's width from the interval
    // The carry from those nodes to the interval's 64 is a FIXED matrix in the interval's own coordinate, while both node sets are
    // doubles near nu: a sample taken half an ulp(nu) from its ideal place is off by 2 (ulp / 2) / distance of a 1/dnu^2 wing, and
    // nothing downstream knows (the 64-node sums go through matrices built from the stored nodes themselves, and the tile nodes of
    // k_voigt_edge_mx likewise).  Fewer nodes only where ulp / distance <= 8e-14 (cut-off 25 cm^-1 at 2500 cm^-1: 2.4e-14 / 3.7e-14;
    // a cut-off of 1 cm^-1 there would give 9e-13 -- tests/test_gpu_fuzz.py::test_interp_fuzz[8] once the short grids took this path)
    const double ulp_hi = std::nextafter(std::fabs(nu[nnu - 1]), INFINITY) - std::fabs(nu[nnu - 1]);
    for (int l = 0; l < g.nlev; l++) {
        gi.nfar[l] = (l > gi.l0 && g.span[l - 1] > 0.0 && g.span[l] > 0.0) ? far_node_count(cut - g.span[l - 1], 0.5 * g.span[l]) : CS_NC;
        if (gi.nfar[l] < CS_NC && !(ulp_hi <= 8e-14 * (cut - g.span[l - 1]))) gi.nfar[l] = CS_NC;
        if (ds > 0.0) gi.nfar[l] = CS_NC;   // (a shifted group's far pieces are not at the distance far_node_count was given)
    }
    for (int l = 0; l < g.nlev; l++) {
        std::vector<WaveWin> iwin;
        wave_windows(nul, g0, g1, nu, nnu, cut, iwin, g.itv[l], ds);
        if ((rc = upload(gi.iwin[l], iwin.data(), iwin.size(), s))) return rc;
        HIPCHK(hipStreamSynchronize(s));   // iwin is a local
    }
    HIPCHK(gi.iz.reserve((size_t)K * g.nItot * sizeof(IZone)));
    HIPCHK(gi.sep.reserve((size_t)((K + 15) / 16) * g.nItot * sizeof(SepZone)));
    HIPCHK(gi.edge.reserve((size_t)((K + 15) / 16) * (size_t)((nnu + 63) / 64) * sizeof(EdgeZone)));
    if (own_F && gi.F.bytes < (size_t)g.nItot * CS_NC * cheb_kpad(K) * sizeof(double)) {
        HIPCHK(gi.F.reserve((size_t)g.nItot * CS_NC * cheb_kpad(K) * sizeof(double)));
        HIPCHK(hipMemsetAsync(gi.F.p, 0, gi.F.bytes, s));   // padding states stay finite
    }
    return CS_OK;
}

Interp interp_view(const ChebGrid &g, const GasInterp &gi, int K, IZone *iz_override = nullptr)
{
    Interp v;
    v.nlev = gi.nlev;
    v.l0 = gi.l0;
    v.nItot = g.nItot;
    v.Kpad = cheb_kpad(K);
    v.nodes = g.nodes.as<double>();
    v.iz = iz_override ? iz_override : gi.iz.as<IZone>();
    v.F = gi.F.as<double>();
    v.sep = gi.sep.as<SepZone>();
    v.edge = gi.edge.as<EdgeZone>();
    if (g.tile_nodes_ok) { v.tnodes = g.tnodes.as<double>(); v.tC = g.tC.as<double>(); }
    for (int l = 0; l < gi.nlev; l++) {
        v.itv[l] = g.itv[l]; v.nI[l] = g.nI[l]; v.ioff[l] = g.ioff[l];
        v.nfar[l] = gi.nfar[l];
        v.Cm[l] = g.Cm[l].as<double>();
        v.Rc[l] = g.Rc[l].as<double>();
        v.iwin[l] = gi.iwin[l].as<WaveWin>();
    }
    return v;
}

void launch_apply(hipStream_t s, const ChebApply &A, int Kpad, int64_t nnu, int kn, double base, const double *extra, double *sigma,
                  int accumulate, bool varnc = false);
// the node sums of ONE F (levels l0 ..) to the grid: level by level into the next smaller one, then the smallest (k_cheb_cascade), or
// every level by itself
// (measured: five levels, BASELINE configs[4]: apply 1.31 -> 1.12 ms; three levels, the bench column: 0.092 -> 0.100 ms, a 1/8 shard
//  of it 0.029 -> 0.037 ms -- F goes through memory once more per level, and each level is one more launch)
static bool cascade_pays(int nlevels_in_use) { return nlevels_in_use >= 4; }
void launch_apply_cascade(hipStream_t s, ChebApply A, const double *const *Rc, const int *itv, const int *nI, int mode, int Kpad, int64_t nnu,
                          int kn, double base, const double *extra, double *sigma, int accumulate, ChebApply *carry = nullptr /* != NULL: the
                          cascade only; *carry = what is still to be carried to the grid (k_flux does that) */)
{
    const int l0 = A.l0[0];
    const bool on = A.ngas == 1 && A.nlev - l0 >= 2 && mode != 2 && (mode == 1 || cascade_pays(A.nlev - l0));
    if (on) {
        const int nst = cheb_kpad(kn) / 16;
        double *F = const_cast<double *>(A.F[0]);
        for (int l = l0 + 1; l < A.nlev; l++) {
            int pshift = 0;
            for (int r = itv[l - 1] / itv[l]; r > 1; r >>= 1) pshift++;
            CS_LAUNCH(k_cheb_cascade, dim3((unsigned)(((int64_t)nI[l] * nst + 3) / 4)), dim3(256), 0, s, Rc[l], F, A.ioff[l - 1], A.ioff[l], pshift,
                      nI[l], Kpad, nst);
        }
        A.l0[0] = A.nlev - 1;
    }
    if (carry) { *carry = A; return; }
    launch_apply(s, A, Kpad, nnu, kn, base, extra, sigma, accumulate);
}
void launch_apply(hipStream_t s, const ChebApply &A, int Kpad, int64_t nnu, int kn, double base, const double *extra, double *sigma,
                  int accumulate, bool varnc)
{
    const int nt64 = (int)((nnu + 63) / 64);
    const int kp = cheb_kpad(kn);                // sub-tiles actually in use (Kpad is the row pitch of F)
    const int nst = kp / 16;
    const unsigned tb8 = (unsigned)(((nt64 + 3) / 4 + 7) / 8 * 8);
    (void)Kpad;
#ifndef CS_APPLY_NSUB
#define CS_APPLY_NSUB 2
#endif
    const bool big = (int64_t)nt64 * ((nst + CS_APPLY_NSUB - 1) / CS_APPLY_NSUB) >= 2048;   // enough (tile, state chunk) waves to fill 1024 SIMDs twice
    const dim3 gridb(tb8 * (unsigned)((nst + CS_APPLY_NSUB - 1) / CS_APPLY_NSUB)), grids(tb8 * (unsigned)nst);
    if (varnc) {
        if (big) CS_LAUNCH((k_cheb_apply_mfma<CS_APPLY_NSUB, true>), gridb, dim3(256), 0, s, A, Kpad, nnu, nt64, kn, base, extra, sigma, accumulate);
        else CS_LAUNCH((k_cheb_apply_mfma<1, true>), grids, dim3(256), 0, s, A, Kpad, nnu, nt64, kn, base, extra, sigma, accumulate);
    } else {
        if (big) CS_LAUNCH((k_cheb_apply_mfma<CS_APPLY_NSUB, false>), gridb, dim3(256), 0, s, A, Kpad, nnu, nt64, kn, base, extra, sigma, accumulate);
        else CS_LAUNCH((k_cheb_apply_mfma<1, false>), grids, dim3(256), 0, s, A, Kpad, nnu, nt64, kn, base, extra, sigma, accumulate);
    }
}

// PHCO2 fast path preconditions.  Returns false -> generic kernel.
static bool phco2_fast_ok(const GasTable &G, const PhGrid &g, double cut)
{
    if (cut < 130.0 || g.nnu < 2 || !(g.nu_hi > g.nu_lo)) return false;
    // widest near zone of any state must stay inside the chi = 1 core (|dnu| < 3 cm^-1) of its tile
    const double amax = ((g.nu_hi + cut) / kC) * std::sqrt(2.0 * kRgas * kTmax / G.mu_min);
    if (100.0 * amax / kSqLn2 * (1.0 + 1e-6) > 2.9) return false;
    if ((g.nu_hi - g.nu_lo) / (double)(g.nnu - 1) * 64.0 > 5.0) return false;   // (mean tile span: wider tiles would not be faster)
    if (!(g.max_span <= 27.0)) return false;   // k_phco2's boundary sets hold one region boundary each: no tile wider than 30 - 3 cm^-1
    // the tabulated line factors exp(+-b_r (nul - nu_c)) must stay in range: b_r <= 0.0888
    if (0.0888 * (0.5 * (g.nu_hi - g.nu_lo) + cut) > 600.0) return false;
    return true;
}
// names a grid: one per column setup and per gas_states call (PhGrid::id)
static std::atomic<uint64_t> g_grid_counter{0};
// interpolation levels of the PHCO2 far wings on that grid with the regions of `drop` (ph_wide_regions) kept out; vl.nv == 0: none (k_phco2
// sums every pair per point).  Reads its arguments only: ph_key of the same four names what the result was formed from.
static PhLevelSet ph_levels(const PhGrid &grid, const PhRules &rules, double cut, int drop)
{
    PhLevelSet g;
    const int64_t nnu = grid.nnu;
    memset(&g.lv, 0, sizeof g.lv);
    memset(&g.vl, 0, sizeof g.vl);
    for (int r = 0; r < 3; r++) { g.fine.off[r] = -1; g.fine.shift[r] = 0; }
    g.nnodes = g.nslots = 0;
    if (!rules.itp_on || nnu < 128) return g;
    const double dnu = (grid.nu_hi - grid.nu_lo) / (double)(nnu - 1);
    // (cs_set_interp_plan's limits of 128 and 2048 points are the Voigt path's; left there, the wide PHCO2 window also takes 4096 and
    //  8192 points; Settings::ph_nodes bit 1: also the tiles themselves as 64-point intervals with 16 or 32 nodes -- measured a tie at C3 size: 1.2 ms
    //  more in k_phco2_nodes, whose smallest waves are a chain of short batches, for 1.3 ms less in k_phco2)
    const int szmax = rules.itp_max >= 2048 ? 8192 : rules.itp_max, szmin = (rules.itp_min <= 128 && (rules.nodes & 2)) ? 64 : rules.itp_min;
    const double Dn[3] = {3.0, 30.0, 120.0}, Df[3] = {30.0, 120.0, cut};
    int need[8][3];   // per size and region: node count, 0 = not carried
    int nreal = 0, real_of[8];
    for (int i = 0; i < 8; i++) {
        const int sz = 8192 >> i;
        real_of[i] = -1;
        if (!(sz <= szmax && sz >= szmin && 2.3 * sz * dnu <= 1.5 * cut && sz / 2 <= nnu && sz * dnu > 1e-8 * std::fabs(grid.nu_hi))) continue;
        const double span = grid.lev_span[i], h = 0.5 * span;
        bool any = false;
        for (int r = 0; r < 3; r++) {
            const double dn = std::max(Dn[r], rules.margin * h);
            need[i][r] = 0;
            if ((drop >> r) & 1) continue;                                  // a state too wide for this region's interpolation (ph_wide_regions)
            if (!(Df[r] - dn - sz * dnu >= 0.05 * (Df[r] - Dn[r]))) continue;   // (next to) nothing to hold at this size
            const double x0 = 1.0 + std::max(Dn[r] / h, rules.margin), lr = std::log10(x0 + std::sqrt(x0 * x0 - 1.0));
            need[i][r] = (rules.nodes & 1) ? 64 : (15.0 * lr >= 18.0 ? 16 : (31.0 * lr >= 18.0 ? 32 : 64));
            any = true;
        }
        if (!any) continue;
        real_of[i] = nreal;
        g.lv.itv[nreal] = sz;
        g.lv.nI[nreal] = (int)((nnu + sz - 1) / sz);
        g.lv.ioff[nreal] = g.lv.nItot;
        g.lv.nItot += g.lv.nI[nreal];
        nreal++;
    }
    g.lv.nlev = nreal;
    if (nreal == 0) return g;
    // virtual levels; more than CS_MAX_ALEVEL of them: the regions of a size join its larger node count
    for (;;) {
        int nv = 0;
        for (int i = 0; i < 8; i++) {
            if (real_of[i] < 0) continue;
            for (int nc = 64; nc >= 16; nc >>= 1) {
                int mask = 0;
                for (int r = 0; r < 3; r++) if (need[i][r] == nc) mask |= 1 << r;
                if (mask) nv++;
            }
        }
        if (nv <= CS_MAX_ALEVEL) break;
        bool changed = false;
        for (int i = 7; i >= 0 && !changed; i--)
            for (int r = 0; r < 3 && !changed; r++)
                if (real_of[i] >= 0 && need[i][r] > 0 && need[i][r] < 64) { need[i][r] *= 2; changed = true; }
        if (!changed) break;
    }
    int nv = 0, last[3] = {-1, -1, -1};   // last[r]: the size above that carries region r
    for (int i = 0; i < 8; i++) {
        if (real_of[i] < 0) continue;
        for (int nc = 64; nc >= 16; nc >>= 1) {
            int mask = 0;
            for (int r = 0; r < 3; r++) if (need[i][r] == nc) mask |= 1 << r;
            if (!mask || nv >= CS_MAX_ALEVEL) continue;
            g.vl.rl[nv] = real_of[i]; g.vl.nc[nv] = nc; g.vl.rmask[nv] = mask;
            g.vl.noff[nv] = g.nnodes; g.vl.boff[nv] = g.nslots;
            for (int r = 0; r < 3; r++) g.vl.par[nv][r] = last[r];
            g.nnodes += g.lv.nI[real_of[i]] * nc;
            g.nslots += g.lv.nI[real_of[i]];
            nv++;
        }
        for (int r = 0; r < 3; r++)
            if (need[i][r] > 0) {
                last[r] = real_of[i];
                g.fine.off[r] = g.lv.ioff[real_of[i]];
                g.fine.shift[r] = 0;
                for (int x = (8192 >> i) / 64; x > 1; x >>= 1) g.fine.shift[r]++;
            }
    }
    g.vl.nv = nv;
    g.vl.boff[nv] = g.nslots;
    return g;
}
// The node counts of ph_levels take the line centre, max(D_r, margin h) away, for the nearest singularity of a line's term.  The term's
// denominator x^2 + (chi y)^2 vanishes where d = nu - nul = +-i gamma chi_r(d), chi_r(d) = exp(a_r - b_r d): |d| = gamma exp(a_r - b_r Re d)
// and arg d = pi/2 - b_r Im d.  For a narrow line these are the Lorentzian's own poles, +-i gamma beside the centre; for a wide one the
// phase b_r Im d turns them towards the real axis -- at 25 K and 3e6 Pa (gamma = 12 cm^-1, chi up to 4.5 since B1 < 0 below 143.6 K) one
// sits 35 cm^-1 from the centre and 20 above the axis, over the region-2 set of a 2048-point interval, whose 32 nodes then leave 5e-12
// (measured: tests/test_gpu_phco2_line.py).  With G_r = gamma max(e^(a_r), e^(a_r - 2 b_r D_far)) bounding |d| for 0 <= Re d <= 2 D_far
// (the larger end of a monotone function), Re d = |d| sin(b_r Im d) <= G_r sin(min(|b_r| G_r, pi/2)): a region is interpolated only while
// that reach stays below a tenth of its near distance D_r for every state of the launch (the 18 digits ph_levels asks for keep 16 with the
// distance 10 % short); else k_phco2 sums its lines per point.  Returns the regions to drop (bit r).
int ph_wide_regions(const double *T, const double *gmax, int64_t n, double cut)
{
    int drop = 0;
    const double Dn[3] = {3.0, 30.0, 120.0}, Df[3] = {30.0, 120.0, cut};
    for (int64_t k = 0; k < n; k++) {
        const double B1 = 0.0888 - 0.16 * std::exp(-0.0041 * T[k]), B2 = 0.0526 * std::exp(-0.00152 * T[k]), B3 = 0.0232;
        const double a[3] = {3.0 * B1, -27.0 * B1 + 30.0 * B2, -27.0 * B1 - 90.0 * B2 + 120.0 * B3}, b[3] = {B1, B2, B3};
        for (int r = 0; r < 3; r++) {
            const double G = gmax[k] * std::exp(std::max(a[r], a[r] - 2.0 * b[r] * Df[r]));
            const double reach = G * std::sin(std::min(std::fabs(b[r]) * G, 1.5707963267948966));
            if (!(reach <= 0.1 * Dn[r])) drop |= 1 << r;
        }
    }
    return drop;
}

// points per sub-tile of k_voigt_sub (16: 0.34 ms at C3 with every core on the 8-term series; 8: 0.22; 4: 0.22 -- what is left is not
// the evaluations)
constexpr int CS_SUBW = 8;
// per-point matrix pieces only on tables with at least this many lines per tile in range (C5: the synthetic O3 table at 6.4 per
// tile gains 0.12 ms with them, the HITRAN fixtures at 0.4-0.7 lose)
constexpr int CS_EDGE_DENS = 4;

// matrix-core node sums (k_cheb_nodes_mx): fp64 Voigt and Lorentz, and by default only where there are enough (interval, state group)
// blocks to fill the chip -- on a short grid (a nu-shard) the one-state-per-wave vector kernel has the shorter critical path
// (1/8 of C3: 0.17 vs 0.25 ms)
static bool mx_big(int nblocks, int kn, int min_blocks) { return (int64_t)nblocks * ((kn + 15) / 16) >= min_blocks; }
// `small`: Settings::small_mx -- short grids too, through the variants that share one (interval | tile, group) between the four
// waves of a block (k_cheb_nodes_mx with every level split, k_voigt_edge_mx<4>)
static bool sep_in_use(bool have_sep, bool always, int nblocks_intervals, int kn, bool mixed, bool small = false)
{
    (void)mixed;   // (the mixed-precision variant keeps the matrix-core pieces in fp64: only the vector bodies beyond far_s go to fp32)
    return have_sep && (always || small || mx_big(nblocks_intervals, kn, 2048));
}
// the per-point pieces (k_voigt_edge_mx: one wave per (tile, state group), no reduction) pay on shorter grids -- 1/4 of C3 (1564
// waves): far 0.42 -> 0.36 ms; 1/8: 0.261 -> 0.244 ms, which the extra zone launch eats -- but only on tables dense enough to give
// a wave more than a few steps (C5's HITRAN fixtures: far 3.94 -> 4.01 ms with them; its synthetic O3 table: step 10.63 -> 10.51)
static bool edge_in_use(bool have_edge, bool always, int ntiles, int kn, bool mixed, int64_t lines_in_range, bool small = false)
{
    (void)mixed;
    return have_edge && (always || ((small || mx_big(ntiles, kn, 1024)) && lines_in_range >= (int64_t)ntiles * CS_EDGE_DENS));
}

// Short grids (a nu-shard): the kernels no longer fill the chip, a step is a chain of launch tails -- and the node sums (F) and the
// per-point kernels (sigma) of a group are independent until the interpolation carries F to the grid.  With a Fork the node kernels
// go to a side stream behind an event recorded after k_gas_setup / k_mxzones; `pending` says the main stream has not yet waited
// for them (it must before anything reads F or overwrites the records).
struct Fork {
    bool use_nodes, use_near;   // which of the two side streams this step uses
    hipStream_t s2; hipEvent_t ev_fork, ev_join; bool pending;
    // the same for the near-line kernels: they need the hand-off words of k_voigt_far / k_voigt_sub and nothing of k_voigt_edge_mx --
    // a gather-bound kernel beside a matrix-core one -- but both add to sigma, so the near-line pairs go to a plane of their own
    // (sigma2: cleared at the start of the step's first Voigt group, read together with sigma by k_rt, folded in by k_fold where sigma is
    // the result).  k_voigt_sub goes there too: it needs the zones only, not k_voigt_far, so it runs beside it.
    hipStream_t s3; hipEvent_t ev_fork3, ev_join3, ev_far3; bool pending3;
    double *sigma2; bool zeroed, live;
};
static void fork_join(Fork *f, hipStream_t s, bool nodes = true, bool near = true)
{
    if (f && nodes && f->pending) { (void)hipStreamWaitEvent(s, f->ev_join, 0); f->pending = false; }
    if (f && near && f->pending3) { (void)hipStreamWaitEvent(s, f->ev_join3, 0); f->pending3 = false; }
}

// One pass of one launch group over kn states: K1 (parameters), K2 (the line sum into sigma [kn][nnu]) and the step that finishes shape
// codes 4, 5 and 6 behind it (launch_gas).  A caller states facts -- the group's final plane, whether it accumulates, base, extra,
// clamp, the spare plane -- and launch_gas decides what the line sum of such a group is given and what follows it.  Views only: nothing
// here owns memory.
struct GasPass {
    // the table, its record range and the shape
    const GasTable *G = nullptr;
    int shape = SH_VOIGT;           // of the line sum: codes 4, 5, 6 are SH_VOIGT with ped / vvh
    int64_t jlo = 0, jhi = 0;       // only the lines some window can reach (windows are sorted: first tile's start .. last tile's end)
    double cut = 25.0;
    bool ped = false;               // shape codes 4, 6, 7: the pedestals of the included lines [pa, pb) come off behind the line sum
    bool vvh = false;               // shape codes 5, 6, 7: every Voigt kernel, over records of S / R(nul, T) (k_gas_setup*_vvh); then R(nu, T) and
    int64_t pa = 0, pb = 0, mb = 0; // the mirror term of the lines [pa, mb) (vvh_mirror_end)
    // CS_SHAPE_PSHIFT (codes 0-2) and shape code 7 (with ped and vvh): records centred at nul + delta_a P / P0, lines whose shifted centre fails the strict pre-filter (flo, fhi)
    // parked.  Every kernel reads the record's centre for the values and the cut-off tests; what is decided from TABLE positions -- the
    // windows and zones of the tiles, the interval zones of the interpolated wings, J0 / J1 and the record range -- was (caller) or is
    // (zones: ZoneArgs::ds) widened by the group's largest shift ds.  Off for such groups: the fp32 wings (far_term32 reads the table
    // position) and the matrix-core pieces (their 1/dnu^2 operand is formed from table positions, state-independent)
    bool pshift = false;
    double flo = -INFINITY, fhi = INFINITY, ds = 0.0;
    // the states
    int kn = 0;
    const double *Tk = nullptr, *Pk = nullptr, *Ppk = nullptr, *scale = nullptr;
    int mstride = 0;                // members of a merged table: element (m, k) of Ppk / scale at m * mstride + k
    const double *lrt = nullptr, *qrefq = nullptr;   // state_tables(): [kn], [kn][niso]
    const double *gbound = nullptr; // [kn] largest Lorentz width (gamma_bound)
    const double *h_Tk = nullptr, *h_gbound = nullptr;   // host copies of Tk and gbound (NULL: none kept -- PHCO2 then interpolates no region)
    // the grid and its windows
    const double *dnu = nullptr, *nu = nullptr;      // on the device, on the host
    int64_t nnu = 0;
    int ntile256 = 0;
    const int32_t *J0 = nullptr, *J1 = nullptr;      // the line kernels' windows of the 256-point tiles (tile_windows)
    const WaveWin *win = nullptr;
    int xtiles = 0;                 // longest XCD stretch of the far kernel's tile order, in tiles (wave_windows)
    // the workspace
    LineHot *hot = nullptr;
    LineCold *cold = nullptr;
    LineF32 *hot32 = nullptr;       // fp32 records of the far wings beyond far_s (mixed precision); NULL: fp64 throughout
    Zone *zones = nullptr;
    unsigned *ranges = nullptr;     // the near-line hand-off (NearHandoff)
    double *ped_ws = nullptr;       // ped_bytes(kn, G->L) where ped
    // the output: sigma = (accumulate ? sigma : base + extra) + this group, then max(0, .) if clamp (codes 4, 6 where the gas's own sigma
    // is complete: B1, bake)
    double base = 0.0;
    const double *extra = nullptr;
    double *sigma = nullptr;        // the group's final plane
    int accumulate = 0;
    bool clamp = false;
    double *spare = nullptr;        // the line sum of a code-5/6 group that accumulates goes here first (one that does not: sigma itself)
    // how to run
    double far_s = 1e6;
    const Settings *set = &kDefaultSettings;   // the lab switches this pass runs under (see kDefaultSettings for who follows the context)
    bool fuse_apply = false;        // the column's only interpolating group, under Settings::fuse_apply: k_voigt_edge_mx may carry the node sums to the grid itself
    Interp itp;
    ChebApply *defer = nullptr;
    PhScratch *ph = nullptr;
    Fork *fork = nullptr;
    hipEvent_t *evg = nullptr;      // NULL or 6 events: after K1 (+ zones), nodes (vector unit), nodes (matrix cores), far (vector unit), sub-tile cores, far (matrix cores)
    bool records_ready = false;     // hot / cold already hold this gas at these states: zones and sums only
    // what the caller wants to know afterwards
    StepLog *log = nullptr;         // the record of the step this pass belongs to (NULL: none kept)
    VoigtPlan *keep = nullptr;      // where the plan of a Voigt / Lorentz group is kept (NULL: nowhere)
};

static ZoneArgs zone_args(const GasPass &p, bool lor, double margin, double ds)
{
    ZoneArgs za;
    za.nu = p.dnu; za.nul = p.G->nu.as<double>(); za.Tk = p.Tk; za.gbound = p.gbound; za.win = p.win; za.zones = p.zones; za.nnu = p.nnu;
    za.lorentz = lor ? 1 : 0;
    za.ntile = (int)((p.nnu + 63) / 64); za.K = p.kn; za.mu_min = p.G->mu_min; za.mu_max = p.G->mu_max; za.cut = p.cut; za.far_s = p.far_s;
    za.margin = margin;
    za.ds = ds;
    return za;
}

// k_voigt_far as launched: fp32 wings or not, 1 / 2 / 4 waves per tile, and the Lorentz body, or the window ends left to k_voigt_edge_mx, or neither
using FarKernel = decltype(&k_voigt_far<false, 1, false, false>);
template <bool MIX, bool LOR, bool EDGE> static FarKernel far_kernel_split(int split)
{
    return split == 1 ? k_voigt_far<MIX, 1, LOR, EDGE> : (split == 2 ? k_voigt_far<MIX, 2, LOR, EDGE> : k_voigt_far<MIX, 4, LOR, EDGE>);
}
static FarKernel far_kernel(bool mixed, int split, bool lor, bool edge)
{
    if (lor) return edge ? far_kernel_split<false, true, true>(split) : far_kernel_split<false, true, false>(split);
    if (mixed) return edge ? far_kernel_split<true, false, true>(split) : far_kernel_split<true, false, false>(split);
    return edge ? far_kernel_split<false, false, true>(split) : far_kernel_split<false, false, false>(split);
}

// How a Voigt / Lorentz group of this pass is run.  Host arithmetic only: launches nothing, reads no device data.
static VoigtPlan voigt_plan(const GasPass &p)
{
    const Interp &itp = p.itp;
    const Settings &st = *p.set;
    const int kn = p.kn;
    const int64_t nlines = std::max(p.jhi, p.jlo) - p.jlo;   // the lines some window can reach
    const bool mixed = p.shape == SH_VOIGT && !p.pshift && p.hot32 != nullptr;   // (no fp32 wings for shifted lines, nor a Lorentz variant)
    VoigtPlan pl;
    memset(&pl, 0, sizeof pl);
    pl.lor = p.shape == SH_LORENTZ;
    pl.nt64 = (int)((p.nnu + 63) / 64);
    pl.ngrp = (kn + 15) / 16;
    // wave priority of the near-line stream's kernels (wave_prio): long grids only
    pl.near_prio = (st.near_prio == 2 || (st.near_prio == 0 && pl.nt64 >= 512)) ? 3 : 0;
    pl.sub_lean = st.sub_lean;
    pl.nb_zones = (unsigned)(((int64_t)pl.nt64 * kn + 255) / 256);
    if (itp.nlev > 0) {
        pl.q0 = itp.ioff[itp.l0];
        for (int r = itp.itv[itp.nlev - 1] / 64; r > 1; r >>= 1) pl.ishift++;
        const int nq = itp.nItot - pl.q0;
        pl.nb_iz = (unsigned)(((int64_t)nq * kn + 255) / 256);
        // what the matrix cores take of the interpolated sets and of the window ends (not of a shifted group: GasPass::pshift)
        if (!p.pshift) {
            pl.use_sep = sep_in_use(itp.sep != nullptr, st.matrix_nodes == 2, nq, kn, mixed, st.small_mx);
            pl.use_edge = edge_in_use(itp.edge != nullptr, st.matrix_nodes == 2, pl.nt64, kn, mixed, nlines, st.small_mx);
        }
        // short grids: four waves per (interval, state) (Settings::nodes_split: 0 = below 16384 waves, 1 = always, 2 = never)
        pl.nsplit4 = st.nodes_split == 1 || (st.nodes_split == 0 && (int64_t)nq * kn < 16384);
        if (pl.use_sep) {
            // the largest interval sizes in use are shared by the four waves of a block -- Settings::nsplit_levels of them (all sizes on a
            // grid too short to fill the chip with one (interval, group) per wave)
            for (int l = itp.l0; l < std::min(itp.nlev, itp.l0 + st.nsplit_levels); l++) pl.nsplit += itp.nI[l];
            if (!mx_big(nq, kn, 2048) || pl.nsplit > nq) pl.nsplit = nq;
            pl.nblk_mx = (unsigned)(pl.nsplit * pl.ngrp) + (unsigned)(((int64_t)(nq - pl.nsplit) * pl.ngrp + 3) / 4);
            pl.far_R = itp.R != nullptr && !(st.far64_shared && pl.nsplit == nq);
            pl.far64_shared = itp.R != nullptr && !pl.far_R;
            for (int l = 0; l < itp.nlev; l++) pl.nfar[l] = itp.nfar[l] > 0 ? itp.nfar[l] : CS_NC;
        }
    }
    pl.core = pl.use_edge && st.matrix_core && !pl.lor;   // (a Lorentz group takes no cores: the lines within the 4-term radius of a tile stay with k_voigt_far's exact body)
    // The piece tables per (interval | tile, state group) need the zones -- which their sixteen-lanes-per-item form computes itself, as
    // blocks of the SAME launch (k_gas_setup_mx); the one-thread-per-item form reads them, a launch of its own behind k_gas_setup
    if (pl.use_sep || pl.use_edge) {
        const int64_t nsep = pl.use_sep ? (int64_t)(itp.nItot - pl.q0) * pl.ngrp : 0, nedge = pl.use_edge ? (int64_t)pl.nt64 * pl.ngrp : 0;
        // sixteen lanes per item shorten the chain where the items are few (a nu-shard: 21 -> 8 us; the bench column 27 -> 9); from
        // ~50 000 items on one thread per item has parallelism enough and sixteen times fewer threads (BASELINE configs[4]: 0.256 vs 0.276 ms)
        const bool one_thread = st.tables_one_thread || nsep + nedge > 50000;
        // merged on short grids, where the head of the step is a chain of launch tails (1/8 of the bench column: 0.347 -> 0.340 ms);
        // at full size the second set of searches beside 300 MB of record stores costs more than the launch it saves (1.900 -> 1.908)
        // (Settings::tables_merge: 1 = never, 2 = always, A/B)
        const bool merged = !one_thread && st.tables_merge != 1 && (st.tables_merge == 2 || pl.nt64 < 1024);
        pl.tables = one_thread ? TABLES_ONE_THREAD : (merged ? TABLES_MERGED : TABLES_LANES16);
        const int per = one_thread ? 256 : 16;   // items per block
        pl.nb_sep = (unsigned)((nsep + per - 1) / per);
        pl.nb_edge = (unsigned)((nedge + per - 1) / per);
    }
    // k_voigt_far, waves per tile: enough waves to fill 256 CUs x 32 wave slots about 4 times over
    const int64_t nwave = (int64_t)pl.nt64 * kn;
    pl.far_split = nwave >= 16384 ? 1 : (nwave >= 4096 ? 2 : 4);   // (re-tuned with the far wings interpolated: waves are 3x shorter)
    if (st.far_split == 1 || st.far_split == 2 || st.far_split == 4) pl.far_split = st.far_split;   // (A/B)
    // k_voigt_edge_mx: one wave per (tile, state group) where those fill the chip, else four (short grid) -- and no tile nodes in that
    // shared form (the 16-node path there: 16 more matrix steps per WAVE, no gain measured)
    pl.edge_big = mx_big(pl.nt64, kn, 1024);
    pl.edge_phases = st.edge_full ? 0 : 1;
    pl.tnodes = pl.use_edge && pl.edge_big && pl.edge_phases && itp.tnodes != nullptr;
    // near kernels: one wave = nrep consecutive tiles, one after the other: eight where the table is sparse against the grid (few tiles have candidates at all) and the
    // grid long enough to keep the chip full with an eighth of the waves, and on every grid of half a million (tile, state) waves
    // and more -- there the launch of the waves is what a near-line kernel costs first (BASELINE configs[4]: 7.9e5 waves per
    // tier, step 7.06 -> 6.85 ms with eight tiles per wave; the bench column, 9.5e4 waves: a tie with two, a loss with four)
    const int64_t nwaves_near = (int64_t)pl.nt64 * kn;
    pl.nrep = (nwaves_near >= 524288 || (nlines < (int64_t)pl.nt64 * 2 && nwaves_near >= 262144)) ? 8 : 1;
    pl.near_both = pl.nrep == 1 && !st.near_two_launches;   // (one tile per wave; Settings::near_two_launches: A/B)
    return pl;
}

// K2 on the far-wing machinery (Voigt, and lorentz! with its own exact body): zones, interpolated wings, k_voigt_far, window cores and ends, near-line tiers
static void line_sum_voigt(hipStream_t s, const GasPass &p, const PrepArgs &pa, unsigned nb_prep)
{
    const GasTable &G = *p.G;
    const Interp &itp = p.itp;
    const int kn = p.kn;
    const int64_t nnu = p.nnu;
    LineF32 *const hot32 = pa.hot32;   // (none under CS_SHAPE_PSHIFT, and no fp32 variant of the Lorentz body)
    int accumulate = p.accumulate;
    const VoigtPlan pl = voigt_plan(p);
    if (p.keep) *p.keep = pl;
    const int nt64 = pl.nt64;
    const bool use_sep = pl.use_sep, use_edge = pl.use_edge;
    // the side streams (not while profiling): the node kernels beside what follows them on the main stream; the near-line kernels and
    // the sub-tile cores into their own plane (Voigt only) -- whose first writer of the step defines all of it: k_voigt_sub where it
    // runs (sums where a tile has a core, zeros elsewhere: Settings::near_memset keeps the memset for A/B), else a memset
    const bool nodes_fork = itp.nlev > 0 && p.fork && p.fork->use_nodes && p.defer && !p.evg;
    const bool near_fork = !pl.lor && p.fork && p.fork->use_near && p.fork->sigma2 && p.defer && !p.evg;
    const bool sub_assigns = near_fork && pl.core && !p.fork->zeroed && !p.set->near_memset;
    const bool near_memset = near_fork && !p.fork->zeroed && !sub_assigns;
    if (p.log) p.log->voigt_group(pl, (nodes_fork ? 1 : 0) | (near_fork ? 2 : 0), near_memset);

    const ZoneArgs za = zone_args(p, pl.lor, p.set->margin, p.pshift ? p.ds : 0.0);
    IzParams P;
    memset(&P, 0, sizeof P);
    if (itp.nlev > 0) {
        P.nlev = itp.nlev;
        P.nItot = itp.nItot;
        P.l0 = itp.l0;
        for (int l = 0; l < itp.nlev; l++) { P.itv[l] = itp.itv[l]; P.nI[l] = itp.nI[l]; P.ioff[l] = itp.ioff[l]; P.iwin[l] = itp.iwin[l]; }
    }
    SepArgs sa;
    EdgeArgs ea;
    memset(&sa, 0, sizeof sa);
    memset(&ea, 0, sizeof ea);
    if (pl.tables != TABLES_NONE) {
        sa.nodes = itp.nodes; sa.nul = G.nu.as<double>(); sa.gbound = p.gbound; sa.Tk = p.Tk; sa.iz = itp.iz; sa.out = itp.sep;
        sa.nItot = itp.nItot; sa.q0 = pl.q0; sa.K = kn; sa.ngrp = pl.ngrp; sa.mu_min = G.mu_min; sa.cut = p.cut; sa.min_states = p.set->mx_min_states;
        sa.lorentz = ea.lorentz = pl.lor ? 1 : 0;
        ea.nu = p.dnu; ea.nul = G.nu.as<double>(); ea.gbound = p.gbound; ea.Tk = p.Tk; ea.win = p.win; ea.zones = p.zones;
        ea.iz = itp.iz + itp.ioff[itp.nlev - 1]; ea.out = itp.edge; ea.nnu = nnu; ea.ntile = nt64; ea.K = kn; ea.ngrp = pl.ngrp;
        ea.nI = itp.nItot; ea.ishift = pl.ishift;
        ea.mu_min = G.mu_min; ea.mu_max = G.mu_max; ea.cut = p.cut;
        ea.core = pl.core ? 1 : 0;
        ea.core4 = 0.0;   // (always the 8-term series in the core: measured at C3 with 0.75 / 0.3 / 0 x the tile's span for the 4-term one: 2.61 / 2.55 / 2.52 ms)
    }
    if (pl.tables == TABLES_MERGED)
        CS_LAUNCH(p.vvh ? k_gas_setup_mx_vvh : k_gas_setup_mx, dim3(nb_prep + pl.nb_zones + pl.nb_iz + pl.nb_sep + pl.nb_edge), dim3(256), 0, s, nb_prep, pl.nb_zones, pl.nb_iz, pl.nb_sep, pa, za, P, itp.iz, sa, ea);
    else
        CS_LAUNCH(p.vvh ? k_gas_setup_vvh : k_gas_setup, dim3(nb_prep + pl.nb_zones + pl.nb_iz), dim3(256), 0, s, nb_prep, pl.nb_zones, pa, za, P, itp.iz);
    if (p.evg && itp.nlev == 0) (void)hipEventRecord(p.evg[0], s);
    const IZone *iz = nullptr;
    bool fuse = false;       // k_voigt_edge_mx also applies the interpolated wings (no k_cheb_apply launch for this group)
    ChebApply Afuse;
    memset(&Afuse, 0, sizeof Afuse);
    if (itp.nlev > 0) {   // sigma = base + extra + interpolated far wings; the per-point kernels add the rest
        const int q0 = pl.q0;
        // deferred apply: the gases of a column add their node sums into ONE F (levels an earlier gas has written accumulate)
        const int q_acc = (p.defer && p.defer->ngas > 0 && p.defer->l0[0] < itp.nlev) ? itp.ioff[p.defer->l0[0]] : itp.nItot;
        const bool nsplit4 = pl.nsplit4;
        const dim3 gridn(nsplit4 ? (unsigned)kn * (unsigned)(itp.nItot - q0) : (unsigned)((kn + 3) / 4) * (unsigned)(itp.nItot - q0));
        if (pl.tables == TABLES_ONE_THREAD) CS_LAUNCH(k_mxzones, dim3(pl.nb_sep + pl.nb_edge), dim3(256), 0, s, pl.nb_sep, sa, ea);
        if (pl.tables == TABLES_LANES16) CS_LAUNCH(k_mxzones16, dim3(pl.nb_sep + pl.nb_edge), dim3(256), 0, s, pl.nb_sep, sa, ea);
        if (p.evg) (void)hipEventRecord(p.evg[0], s);
        const SepZone *sepz = use_sep ? itp.sep : nullptr;
        hipStream_t sm = s;   // main stream
        if (nodes_fork) {
            (void)hipEventRecord(p.fork->ev_fork, s);
            (void)hipStreamWaitEvent(p.fork->s2, p.fork->ev_fork, 0);
            s = p.fork->s2;     // the two node kernels below run beside what follows them on the main stream
        }
#define NODES_LAUNCH(M, L_, M4, L4, S4) do { if (nsplit4) CS_LAUNCH((k_cheb_nodes<M4, L4, S4>), gridn, dim3(256), 0, s, itp.nodes, G.L, p.hot, hot32, G.nu.as<double>(), itp.iz, \
                               itp.nItot, q0, q_acc, kn, itp.Kpad, p.cut, itp.F, sepz); \
        else CS_LAUNCH((k_cheb_nodes<M, L_>), gridn, dim3(256), 0, s, itp.nodes, G.L, p.hot, hot32, G.nu.as<double>(), itp.iz, \
                               itp.nItot, q0, q_acc, kn, itp.Kpad, p.cut, itp.F, sepz); } while (0)
        if (pl.lor)
            NODES_LAUNCH(false, true, false, true, 4);
        else if (hot32)
            NODES_LAUNCH(true, false, true, false, 4);
        else
            NODES_LAUNCH(false, false, false, false, 4);
        if (p.evg) (void)hipEventRecord(p.evg[1], s);
        if (use_sep) {
            MxFar mf;
            memset(&mf, 0, sizeof mf);
            mf.nlev = itp.nlev;
            for (int l = 0; l < itp.nlev; l++) { mf.ioff[l] = itp.ioff[l]; mf.nfar[l] = pl.nfar[l]; }
            mf.ioff[itp.nlev] = itp.nItot;
            mf.R = pl.far_R ? itp.R : nullptr;
            CS_LAUNCH(pl.lor ? k_cheb_nodes_mx<true> : k_cheb_nodes_mx<false>, dim3(pl.nblk_mx), dim3(256), 0, s, itp.nodes, G.L, p.hot, itp.sep, itp.nItot, q0, pl.nsplit, kn,
                               itp.Kpad, pl.ngrp, itp.F, itp.iz, mf);
        }
        if (s != sm) {
            (void)hipEventRecord(p.fork->ev_join, s);
            p.fork->pending = true;
            s = sm;
        }
        if (p.evg) (void)hipEventRecord(p.evg[2], s);
        ChebApply A0;
        ChebApply &A = p.defer ? *p.defer : A0;
        if (!p.defer) A.ngas = 0;
        A.nlev = itp.nlev;
        for (int l = 0; l < itp.nlev; l++) {
            A.shift[l] = 0;
            for (int r = itp.itv[l] / 64; r > 1; r >>= 1) A.shift[l]++;
            A.ioff[l] = itp.ioff[l];
            A.nc[l] = CS_NC;
            A.noff[l] = itp.ioff[l] * CS_NC;
            A.Cm[l] = itp.Cm[l];
        }
        fuse = p.defer && p.fuse_apply && use_edge && p.defer->ngas == 0;   // (then k_voigt_edge_mx below carries this group's node sums to the grid)
        if (fuse) {
            Afuse = A;
            Afuse.ngas = 1;
            Afuse.l0[0] = itp.l0;
            Afuse.F[0] = itp.F;
        } else if (p.defer && A.ngas > 0) {
            A.l0[0] = std::min(A.l0[0], itp.l0);   // same F: the sum over the gases so far
        } else {
            A.l0[A.ngas] = itp.l0;
            A.F[A.ngas++] = itp.F;
        }
        if (!p.defer) {   // sigma = base + extra + interpolated far wings now; the per-point kernels add the rest
            launch_apply_cascade(s, A, itp.Rc, itp.itv, itp.nI, p.set->cascade, itp.Kpad, nnu, kn, p.base, p.extra, p.sigma, accumulate);
            accumulate = 1;
        }               // (deferred: the caller applies the node sums of all its gases in one launch, after the last gas)
        iz = itp.iz + itp.ioff[itp.nlev - 1];
    } else if (p.evg) {
        (void)hipEventRecord(p.evg[1], s);
        (void)hipEventRecord(p.evg[2], s);
    }

    const int split = pl.far_split;
    const int nblk_s = (nt64 * split + 3) / 4;
    // 8 x (blocks of the longest XCD stretch): XCD-aware tile mapping (tile_block); xtiles is a multiple of 4 tiles
    const dim3 grid_s((unsigned)(8 * (p.xtiles * split / 4)), kn);
    const EdgeZone *edgez = use_edge ? itp.edge : nullptr;
    // the window cores of the groups whose series radius is short: pairs inside it (the rest: k_voigt_edge_mx)
    auto launch_sub = [&](hipStream_t ss, double *out, bool assigns) {
        CS_LAUNCH(k_voigt_sub<CS_SUBW>, dim3((unsigned)nt64, (unsigned)((kn + 64 / CS_SUBW - 1) / (64 / CS_SUBW))), dim3(4096 / CS_SUBW), 0, ss, p.dnu, nnu, G.L, p.hot,
                  G.nu.as<double>(), p.zones, itp.edge, nt64, kn, p.cut, out, p.ranges, pl.near_prio, assigns ? 1 : 0, pl.sub_lean);
    };
    if (near_fork) {   // zones, records and piece tables are written: the side stream may start
        if (nodes_fork) {   // (nothing was enqueued on the main stream since that record: one event serves both side streams)
            (void)hipStreamWaitEvent(p.fork->s3, p.fork->ev_fork, 0);
        } else {
            (void)hipEventRecord(p.fork->ev_fork3, s);
            (void)hipStreamWaitEvent(p.fork->s3, p.fork->ev_fork3, 0);
        }
        if (near_memset) (void)hipMemsetAsync(p.fork->sigma2, 0, (size_t)kn * nnu * sizeof(double), p.fork->s3);
        p.fork->zeroed = true;
        if (pl.core) launch_sub(p.fork->s3, p.fork->sigma2, sub_assigns);   // (it needs the zones only, not k_voigt_far: beside it)
    }
    CS_LAUNCH(far_kernel(hot32 != nullptr, split, pl.lor, use_edge), grid_s, dim3(256), 0, s, p.dnu, nnu, G.L, p.hot, hot32, G.nu.as<double>(), p.win, kn, p.zones,
              nt64, nblk_s, p.cut, p.base, p.extra, p.sigma, accumulate, p.ranges, iz, itp.nItot, pl.ishift, edgez);
    if (p.evg) (void)hipEventRecord(p.evg[3], s);
    if (pl.core && !near_fork) launch_sub(s, p.sigma, false);
    auto launch_near = [&](hipStream_t sn, double *out) {
        const dim3 gridq((unsigned)(((nt64 + pl.nrep - 1) / pl.nrep + 3) / 4), kn);
        if (pl.near_both) {
            CS_LAUNCH(k_voigt_near_both, gridq, dim3(256), 0, sn, p.dnu, nnu, G.L, p.hot, p.cold, p.zones, nt64, kn, p.cut, out, p.ranges, pl.near_prio);
            return;
        }
        CS_LAUNCH(k_voigt_near<0>, gridq, dim3(256), 0, sn, p.dnu, nnu, G.L, p.hot, p.cold, p.zones, nt64, kn, pl.nrep, p.cut, out, p.ranges, pl.near_prio);
        CS_LAUNCH(k_voigt_near<1>, gridq, dim3(256), 0, sn, p.dnu, nnu, G.L, p.hot, p.cold, p.zones, nt64, kn, pl.nrep, p.cut, out, p.ranges, pl.near_prio);
    };
    if (near_fork) {   // the near kernels need the hand-off words of both k_voigt_far (main stream) and k_voigt_sub (theirs)
        (void)hipEventRecord(p.fork->ev_far3, s);
        (void)hipStreamWaitEvent(p.fork->s3, p.fork->ev_far3, 0);
        launch_near(p.fork->s3, p.fork->sigma2);
        (void)hipEventRecord(p.fork->ev_join3, p.fork->s3);
        p.fork->pending3 = true;
        p.fork->live = true;
    }
    if (p.evg) (void)hipEventRecord(p.evg[4], s);
    if (use_edge) {
        if (fuse) fork_join(p.fork, s);   // (it reads F)
        const unsigned ntx = pl.edge_big ? (unsigned)((nt64 + 3) / 4) : (unsigned)nt64;
        const auto edge_kernel = pl.lor ? (pl.edge_big ? k_voigt_edge_mx<1, true> : k_voigt_edge_mx<4, true>) : (pl.edge_big ? k_voigt_edge_mx<1> : k_voigt_edge_mx<4>);
        CS_LAUNCH(edge_kernel, dim3(ntx, (unsigned)pl.ngrp), dim3(256), 0, s, p.dnu, nnu, G.L, p.hot, p.win,
                  itp.edge, nt64, kn, p.cut, p.sigma, fuse ? 1 : 0, Afuse, itp.Kpad, G.nu.as<double>(), pl.edge_phases,
                  pl.tnodes ? itp.tnodes : (const double *)nullptr, pl.edge_big ? itp.tC : (const double *)nullptr);
    }
    if (p.evg) (void)hipEventRecord(p.evg[5], s);
    if (!pl.lor && !near_fork) launch_near(s, p.sigma);
}

static void launch_line_sum(hipStream_t s, const GasPass &p);

// How the PHCO2 group of this pass is run (p.ph set, the scratch's grid and rules those of the call).  Host arithmetic only: allocates
// nothing, launches nothing; of the scratch it reads grid, rules and the levels built for the same key, and keeps the density answers.
static PhPlan phco2_plan(const GasPass &p)
{
    const GasTable &G = *p.G;
    const PhGrid &g = p.ph->grid;
    const PhRules &rules = p.ph->rules;
    PhPlan pl;
    pl.fast = phco2_fast_ok(G, g, p.cut);
    if (!pl.fast) return pl;
    pl.nt64 = (int)((p.nnu + 63) / 64);
    pl.nb_zones = (unsigned)(((int64_t)pl.nt64 * p.kn + 255) / 256);
    pl.nb_tiles = (unsigned)((pl.nt64 + 255) / 256);
    pl.drop = p.h_Tk && p.h_gbound ? ph_wide_regions(p.h_Tk, p.h_gbound, p.kn, p.cut) : 7;
    pl.key = ph_key(g, rules, p.cut, pl.drop);
    pl.lev = p.ph->key == pl.key ? p.ph->lev : ph_levels(g, rules, p.cut, pl.drop);
    pl.levels = pl.lev.vl.nv > 0;
    if (pl.levels) pl.nb_itv = (unsigned)((pl.lev.lv.nItot + 255) / 256);
    // the pairs within 3 cm^-1 (chi = 1: plain Voigt, every near-line pair among them) through the Voigt kernels, where their
    // near-line hand-off takes this table (check_near_density; else k_phco2's own core loop)
    if (p.ranges && !rules.own_core) {
        std::vector<PhScratch::Dens> &dens = p.ph->dens;
        const PhScratch::Dens *hit = nullptr;
        for (auto &d : dens) if (d.tab == (const void *)&G && d.gen == G.generation && d.grid == g.id) hit = &d;
        if (!hit) {
            if (dens.size() >= 8) dens.erase(dens.begin());
            dens.push_back({(const void *)&G, G.generation, g.id, check_near_density(G, g.nu_hi, g.max_span, 3.0) == CS_OK});
            hit = &dens.back();
        }
        pl.inner = hit->ok;
    }
    return pl;
}

// Reserves what the plan needs on the context's scratch and, where the scratch holds the levels of another key, lays the plan's out in
// their place (their tables are built by the launch: ph_build_levels).  The only place that takes something back from a plan for want of
// memory, silently: without fac / win the group goes to line_sum_generic, without the level buffers k_phco2 sums every pair per point,
// without win3 / zones3 it runs its own core loop.
static void ph_prepare(const GasPass &p, PhPlan &pl)
{
    PhScratch &ph = *p.ph;
    const int kn = p.kn;
    if (!pl.fast) return;
    // a buffer that grows moves, and a captured step of the resident column names the old address (fac, win, win3 and zones3 grow with
    // the states, lines and tiles of any PHCO2 pass, with or without levels): counted like a rebuild, which drops that step's graph
    const void *const held[] = {ph.fac.p, ph.win.p, ph.piw.p, ph.F.p, ph.win3.p, ph.zones3.p};
    struct Moved {
        PhScratch &ph; const void *const *held;
        ~Moved()
        {
            const void *const now[] = {ph.fac.p, ph.win.p, ph.piw.p, ph.F.p, ph.win3.p, ph.zones3.p};
            for (int i = 0; i < 6; i++) if (held[i] && now[i] != held[i]) { ph.builds++; break; }
        }
    } moved{ph, held};
    if (ph.fac.reserve((size_t)6 * kn * p.G->L * sizeof(double)) != hipSuccess || ph.win.reserve((size_t)pl.nt64 * sizeof(PhWin)) != hipSuccess) {
        pl = PhPlan();
        return;
    }
    const bool rebuild = ph.rules.itp_on && !(ph.key == pl.key);
    if (rebuild) {
        ph.key = PhKey();
        ph.builds++;
    }
    if (pl.levels) {
        const size_t fb = (size_t)pl.lev.nnodes * cheb_kpad(kn) * sizeof(double);
        bool ok = !rebuild || ph.nodes.reserve((size_t)pl.lev.nnodes * sizeof(double)) == hipSuccess;
        for (int v = 0; rebuild && ok && v < pl.lev.vl.nv; v++) {
            const int rl = pl.lev.vl.rl[v];
            ok = ph.Cm[v].reserve((size_t)pl.lev.lv.nI[rl] * pl.lev.vl.nc[v] * pl.lev.lv.itv[rl] * sizeof(double)) == hipSuccess;
        }
        ok = ok && ph.piw.reserve((size_t)pl.lev.lv.nItot * sizeof(PhIWin)) == hipSuccess;
        if (ok && ph.F.bytes < fb) {   // (new: cleared once, so that padding states stay finite)
            ok = ph.F.reserve(fb) == hipSuccess;
            pl.clear_F = ok;
        }
        if (!ok) pl.no_levels();
    }
    if (rebuild && (pl.levels || pl.lev.vl.nv == 0)) {   // every buffer held (or no level to hold): the scratch is this key's from here on
        ph.key = pl.key;
        ph.lev = pl.lev;
        pl.build = pl.levels;
    }
    if (pl.inner)
        pl.inner = ph.win3.reserve((size_t)(pl.nt64 + 3) * sizeof(WaveWin)) == hipSuccess && ph.zones3.reserve((size_t)kn * pl.nt64 * sizeof(Zone)) == hipSuccess;
}
// what ph_prepare left to the launch, behind k_gas_setup: the tables of newly laid out levels (nodes and interpolation matrices, one launch
// per virtual level), then the one-time clear of a new F.  Either refused: no levels in this pass, and the next builds them again
static void ph_build_levels(hipStream_t s, const GasPass &p, PhPlan &pl)
{
    PhScratch &ph = *p.ph;
    const PhLevelSet &g = pl.lev;
    for (int v = 0; pl.build && v < g.vl.nv; v++) {
        const int rl = g.vl.rl[v], nc = g.vl.nc[v];
        CS_LAUNCH(k_cheb_setup, dim3(g.lv.nI[rl]), dim3(256), 0, s, p.dnu, p.nnu, g.lv.itv[rl], g.lv.nI[rl], nc, ph.nodes.as<double>() + g.vl.noff[v],
                  ph.Cm[v].as<double>());
    }
    if ((pl.build && hipGetLastError() != hipSuccess) || (pl.clear_F && hipMemsetAsync(ph.F.p, 0, ph.F.bytes, s) != hipSuccess)) {
        ph.key = PhKey();
        if (pl.clear_F) ph.F.release();   // (not cleared: the next pass takes a new one)
        pl.no_levels();
    }
}

// PHCO2 fast path (k_phco2): region-uniform far lines with factorised chi; needs the cut-off edges inside region 3 and the
// near zone inside the chi = 1 core (phco2_fast_ok), else the generic kernel.  Fills the argument structs and launches by the plan.
static void line_sum_phco2(hipStream_t s, const GasPass &p, PrepArgs pa, unsigned nb_prep, PhPlan &pl)
{
    const GasTable &G = *p.G;
    const PhScratch &ph = *p.ph;
    const int kn = p.kn, nt64 = pl.nt64;
    const int64_t nnu = p.nnu, jlo = pa.jlo, jhi = pa.jhi;
    int accumulate = p.accumulate;
    pa.phfac = ph.fac.as<double>();
    pa.nu_c = ph.grid.nu_c;
    const ZoneArgs za = zone_args(p, false, kChebMargin, 0.0);
    IzParams P;
    memset(&P, 0, sizeof P);
    CS_LAUNCH(k_gas_setup, dim3(nb_prep + pl.nb_zones), dim3(256), 0, s, nb_prep, pl.nb_zones, pa, za, P, (IZone *)nullptr);
    if (pl.build || pl.clear_F) ph_build_levels(s, p, pl);
    const PhLevelSet &pg = pl.lev;
    PhArgs pw;
    pw.nu = p.dnu; pw.nul = G.nu.as<double>(); pw.nnu = nnu; pw.ntile = nt64; pw.J0 = (int32_t)jlo; pw.J1 = (int32_t)jhi; pw.cut = p.cut;
    pw.tol = 1e-9 * (std::max(std::fabs(ph.grid.nu_lo), std::fabs(ph.grid.nu_hi)) + p.cut + 1.0);
    pw.out = ph.win.as<PhWin>();
    PhIArgs ia;
    memset(&ia, 0, sizeof ia);
    if (pl.levels) {
        ia.nu = p.dnu; ia.nul = pw.nul; ia.nnu = nnu; ia.J0 = pw.J0; ia.J1 = pw.J1; ia.cut = p.cut; ia.tol = pw.tol; ia.margin = ph.rules.margin;
        ia.lv = pg.lv;
        ia.out = ph.piw.as<PhIWin>();
    }
    WwArgs wa;
    memset(&wa, 0, sizeof wa);
    if (pl.inner) {
        wa.nu = p.dnu; wa.nul = pw.nul; wa.nnu = nnu; wa.ntile = nt64; wa.J0 = pw.J0; wa.J1 = pw.J1; wa.cut = 3.0;
        wa.sparse = (jhi - jlo) * 8 < nnu ? 1 : 0;
        wa.out = ph.win3.as<WaveWin>();
    }
    CS_LAUNCH(k_phwin, dim3(pl.nb_tiles + pl.nb_itv + (pl.inner ? pl.nb_tiles : 0u)), dim3(256), 0, s, pl.nb_tiles, pl.nb_itv, pw, ia, wa);
    if (p.evg) (void)hipEventRecord(p.evg[0], s);
    const PhIWin *piw = nullptr;
    PhFine fine;
    memset(&fine, 0, sizeof fine);
    if (pl.levels) {   // far wings of the region-uniform lines: node sums, carried to the grid (sigma = base + extra + them)
        const int Kpad = cheb_kpad(kn);
        CS_LAUNCH(k_phco2_nodes, dim3((unsigned)pg.nslots * (unsigned)((kn + 3) / 4)), dim3(256), 0, s, ph.nodes.as<double>(), G.L, p.hot,
                  ph.fac.as<double>(), ph.grid.nu_c, ph.piw.as<PhIWin>(), pg.lv, pg.vl, kn, Kpad, p.Tk, p.cut, p.gbound, G.mu_min, G.mu_max, p.far_s,
                  ph.F.as<double>());
        if (p.evg) (void)hipEventRecord(p.evg[1], s);
        ChebApply A;
        memset(&A, 0, sizeof A);
        A.nlev = pg.vl.nv; A.ngas = 1; A.F[0] = ph.F.as<double>(); A.l0[0] = 0;
        for (int v = 0; v < pg.vl.nv; v++) {
            for (int r = pg.lv.itv[pg.vl.rl[v]] / 64; r > 1; r >>= 1) A.shift[v]++;
            A.ioff[v] = pg.vl.boff[v];
            A.nc[v] = pg.vl.nc[v];
            A.noff[v] = pg.vl.noff[v];
            A.Cm[v] = ph.Cm[v].as<double>();
        }
        launch_apply(s, A, Kpad, nnu, kn, p.base, p.extra, p.sigma, accumulate, true);
        accumulate = 1;
        if (p.evg) (void)hipEventRecord(p.evg[2], s);
        piw = ph.piw.as<PhIWin>();
        fine = pg.fine;
    } else if (p.evg) { (void)hipEventRecord(p.evg[1], s); (void)hipEventRecord(p.evg[2], s); }
    CS_LAUNCH(k_phco2, dim3((unsigned)((nt64 + 3) / 4), kn), dim3(256), 0, s, p.dnu, nnu, G.L, p.hot, p.cold, ph.fac.as<double>(), ph.grid.nu_c,
                       ph.win.as<PhWin>(), p.zones, nt64, p.cut, p.Tk, kn, p.base, p.extra, p.sigma, accumulate, piw, fine, pl.inner ? 1 : 0);
    if (p.evg) (void)hipEventRecord(p.evg[3], s);
    if (pl.inner) {
        const int nt4 = (nt64 + 3) / 4 * 4, per = ((nt4 / 4 + 7) / 8) * 4;   // (wave_windows' stretch length)
        GasPass in = p;   // same table, record range, states, records, grid, ranges and plane: the zones and sums of a Voigt pass with its own windows
        in.shape = SH_VOIGT; in.cut = 3.0; in.win = ph.win3.as<WaveWin>(); in.xtiles = per; in.zones = ph.zones3.as<Zone>();
        in.base = 0.0; in.extra = nullptr; in.accumulate = 1; in.evg = nullptr; in.hot32 = nullptr; in.itp = Interp(); in.set = &kDefaultSettings; in.fuse_apply = false;
        in.defer = nullptr; in.ph = nullptr; in.fork = nullptr; in.records_ready = true; in.keep = nullptr;
        in.flo = -INFINITY; in.fhi = INFINITY;   // (no K1 in this pass: nothing reads them)
        launch_line_sum(s, in);
    }
    if (p.log) p.log->phco2_group(pl);   // (the group's far lines were k_phco2's; the inner pass only took the pairs within 3 cm^-1)
    if (p.evg) { (void)hipEventRecord(p.evg[4], s); (void)hipEventRecord(p.evg[5], s); }
}

// every other shape, CS_SHAPE_PSHIFT Doppler and PHCO2 off its fast path: k_linesum over the windows of the 256-point tiles
static void line_sum_generic(hipStream_t s, const GasPass &p, const PrepArgs &pa, unsigned nb_prep)
{
    if (nb_prep > 0) {
        ZoneArgs za;
        IzParams P;
        memset(&za, 0, sizeof za);
        memset(&P, 0, sizeof P);
        CS_LAUNCH(k_gas_setup, dim3(nb_prep), dim3(256), 0, s, nb_prep, 0u, pa, za, P, (IZone *)nullptr);
    }
    if (p.evg) { (void)hipEventRecord(p.evg[0], s); (void)hipEventRecord(p.evg[1], s); (void)hipEventRecord(p.evg[2], s); }
    if (p.log) p.log->line_kernel = 1;
    launch_linesum_shape(p.shape, dim3(p.ntile256, p.kn), s, p.dnu, p.nnu, p.G->L, p.hot, p.cold, p.J0, p.J1, p.cut, p.Tk, p.base, p.extra, p.sigma,
                         p.accumulate);
    if (p.evg) { (void)hipEventRecord(p.evg[3], s); (void)hipEventRecord(p.evg[4], s); (void)hipEventRecord(p.evg[5], s); }
}

// K1 + K2 for one gas on `s`: parameters for `kn` states, then the line sum into sigma ([kn][nnu])
static void launch_line_sum(hipStream_t s, const GasPass &p)
{
    fork_join(p.fork, s);   // (an earlier group's node kernels may still read the records this launch overwrites)
    const GasTable &G = *p.G;
    const int64_t jlo = p.jlo, jhi = std::max(p.jhi, p.jlo);
    PrepArgs pa;
    pa.shape = p.shape; pa.K = p.kn; pa.g = G.dev(); pa.jlo = jlo; pa.jhi = jhi;
    pa.Tk = p.Tk; pa.Pk = p.Pk; pa.Ppk = p.Ppk; pa.scale = p.scale; pa.mstride = p.mstride; pa.lrt = p.lrt; pa.qrefq = p.qrefq; pa.niso = G.niso; pa.hot = p.hot; pa.cold = p.cold;
    pa.hot32 = (p.shape == SH_VOIGT && !p.pshift) ? p.hot32 : nullptr;   // (far_term32 reads the table position: no fp32 wings for shifted lines)
    pa.phfac = nullptr;
    pa.nu_c = 0.0;
    pa.pshift = p.pshift ? 1 : 0; pa.flo = p.flo; pa.fhi = p.fhi;
    const unsigned nb_prep = p.records_ready ? 0u : (unsigned)((jhi - jlo + 255) / 256) * (unsigned)((p.kn + CS_PREP_KC - 1) / CS_PREP_KC);   // (line block, chunk of states)
    if (p.shape == SH_VOIGT || p.shape == SH_LORENTZ) line_sum_voigt(s, p, pa, nb_prep);
    else if (p.shape == SH_PHCO2 && !p.pshift && p.ph) {
        PhPlan pl = phco2_plan(p);
        ph_prepare(p, pl);
        if (pl.fast) line_sum_phco2(s, p, pa, nb_prep, pl);
        else line_sum_generic(s, p, pa, nb_prep);
    } else line_sum_generic(s, p, pa, nb_prep);
}

// workspace of launch_pedestal for kn states of a table of L lines: p, in-block prefix and suffix sums [3][kn][L], block sums [kn][ceil(L / CS_PED_B)]
static size_t ped_bytes(int64_t kn, int64_t L) { return (size_t)kn * ((size_t)3 * L + (L + CS_PED_B - 1) / CS_PED_B) * sizeof(double); }
// ... and its four views
static PedWs ped_views(double *ped_ws, int64_t kn, int64_t L)
{
    const size_t kl = (size_t)kn * L;
    return {ped_ws, ped_ws + kl, ped_ws + 2 * kl, ped_ws + 3 * kl, (L + CS_PED_B - 1) / CS_PED_B};
}

// p and its in-block sums of the included lines [pa, pb) of the group's records, into ws
static void launch_ped_values(hipStream_t s, const GasPass &g, const PedWs &ws)
{
    const int64_t a = g.pa, b = std::max(a, g.pb);
    if (b <= a) return;
    const int64_t q0 = a / CS_PED_B, q1 = (b - 1) / CS_PED_B + 1;
    CS_LAUNCH(k_ped_values, dim3((unsigned)((q1 - q0 + 3) / 4), (unsigned)g.kn), dim3(256), 0, s, g.hot, g.cold, g.G->L, a, b, g.cut, q0, q1 - q0, ws);
}

// shape code 4 behind the group's line sum on the same stream (whose K1 left the Voigt records of these kn states in hot / cold):
// sigma[k][i] -= sum of p[k][l] over the lines l of [pa, pb) with |nu_i - nul_l| <= cut; clamp: then max(0, .) (sigma complete).
// [pa, pb) = the lines the line sum included (the strict end-point pre-filter of the vector method, or every line) within the records'
// range.  ped_ws: ped_bytes(kn, G.L).  Runs before the next group's K1 overwrites the records (stream order).
static void launch_pedestal(hipStream_t s, const GasPass &g)
{
    const GasTable &G = *g.G;
    const PedWs ws = ped_views(g.ped_ws, g.kn, G.L);
    launch_ped_values(s, g, ws);
    CS_LAUNCH(k_ped_sub, dim3((unsigned)((g.nnu + 255) / 256), (unsigned)((g.kn + CS_PED_KC - 1) / CS_PED_KC)), dim3(256), 0, s, g.dnu, g.nnu,
              G.nu.as<double>(), G.L, g.pa, std::max(g.pa, g.pb), g.J0, g.J1, g.cut, g.kn, ws, g.sigma, g.clamp ? 1 : 0);
}

// shape code 5 behind the group's line sum on the same stream, which is in src (base 0, nothing else added; src may be sigma):
// sigma = (accumulate ? sigma : base + extra) + R(nu, T) (src + mirror term of the lines [pa, mb)).
// Reads the records the line sum used: runs before the next group's K1 overwrites them (stream order).
static void launch_vvh(hipStream_t s, const GasPass &g, const double *src)
{
    CS_LAUNCH(k_vvh_finish, dim3((unsigned)((g.nnu + 255) / 256), (unsigned)g.kn), dim3(256), 0, s, g.dnu, g.nnu, g.Tk, g.hot, g.cold, g.G->L, g.pa,
              std::max(g.pa, g.mb), g.cut, src, g.base, g.extra, g.sigma, g.accumulate);
}

// shape code 6 in place of launch_vvh: k_ped_values over the included lines [pa, pb) of the S~ records, then ONE pass k_vvh_ped_finish
// that subtracts each point's direct pedestals, adds the mirror pairs of [pa, mb) minus theirs, multiplies by R(nu, T) and writes
// sigma = (accumulate ? sigma : base + extra) + r, then max(0, .) if clamp.  ped_ws: as launch_pedestal's.
// Shape code 7 (g.pshift): the same k_ped_values over the shifted records, then the SHIFT form of the finish pass, which takes each
// (point, state)'s direct window and mirror lines from the records' own centres; the mirror tiles reach g.ds further.
static void launch_vvh_ped(hipStream_t s, const GasPass &g, const double *src)
{
    const GasTable &G = *g.G;
    const int64_t a = g.pa, b = std::max(a, g.pb), m = std::min(std::max(a, g.mb), b);
    const PedWs ws = ped_views(g.ped_ws, g.kn, G.L);
    launch_ped_values(s, g, ws);
    // the tiles [0, tm) whose first point can reach a mirror line (nu + nul_a <= cut) get one state per block
    const int64_t ntile = (g.nnu + 255) / 256;
    int64_t tm = 0;
    if (m > a) {
        const double lim = g.cut - G.h_nu[a] + (g.pshift ? g.ds : 0.0);
        while (tm < ntile && g.nu[tm * 256] <= lim) tm++;
    }
    const int64_t nblk = tm * g.kn + (ntile - tm) * ((g.kn + CS_PED_KC - 1) / CS_PED_KC);
    // code 7: the windows by the records' own centres (fringes of the table-position window ds wide, with room for the rounding of
    // nul + s and of the searches' differences)
    const double ds = g.pshift ? g.ds + 1e-9 * g.cut : 0.0;
    CS_LAUNCH(g.pshift ? k_vvh_ped_finish<true> : k_vvh_ped_finish<false>, dim3((unsigned)nblk), dim3(256), 0, s, g.dnu, g.nnu, g.Tk,
              G.nu.as<double>(), g.hot, g.cold, G.L, a, b, a, m, g.J0, g.J1, g.cut, ds, g.kn, ws, src, g.base, g.extra, g.sigma, g.accumulate,
              g.clamp ? 1 : 0, (int)tm);
}

// One launch group on `s`, finishing step included.  Codes 0-3: the line sum as the pass states it; code 4: launch_pedestal behind it.
// Codes 5, 6: the bare line sum of the S / R(nul, T) records -- base 0, no extra, applied at once (no deferred apply) and without side
// streams, into sigma itself for a group that does not accumulate, else into the spare plane -- then launch_vvh (5) or launch_vvh_ped
// (6, 7), which write sigma as the pass states it.
static void launch_gas(hipStream_t s, const GasPass &p)
{
    if (!p.vvh) {
        launch_line_sum(s, p);
        if (p.ped) launch_pedestal(s, p);
        return;
    }
    GasPass bare = p;
    bare.base = 0.0; bare.extra = nullptr; bare.sigma = p.accumulate ? p.spare : p.sigma; bare.accumulate = 0;
    bare.defer = nullptr; bare.fork = nullptr;
    launch_line_sum(s, bare);
    if (p.ped) launch_vvh_ped(s, p, bare.sigma);
    else launch_vvh(s, p, bare.sigma);
}

// end of the mirror lines of shape code 5 among the included lines [a, b) whose records exist: nu + nul <= cut can hold for some point
// only where nul <= cut - nu_0 (taken a little wide here: k_vvh_finish applies the exact test).  = a on grids that start at the cut-off
// or above, where k_vvh_finish then only scales.  Code 7: the centre nul + s, |s| <= ds, can reach it from table positions up to ds higher.
static int64_t vvh_mirror_end(const std::vector<double> &nul, int64_t a, int64_t b, double nu0, double cut, double ds)
{
    b = std::max(a, b);
    const double lim = cut - nu0 + ds;
    if (!(lim >= 0.0)) return a;
    return std::upper_bound(nul.begin() + a, nul.begin() + b, lim + 1e-9 * cut) - nul.begin();
}

// a shape code as the entry points take it -- base code 0..7, and CS_SHAPE_PSHIFT ORed onto codes 0, 1, 2 -- taken apart: codes 4, 5, 6, 7
// are the Voigt line sum (line_shape), then the pedestal (ped) and / or R(nu, T) and the mirror term (vvh) behind it; code 7 is code 6 at
// the shifted centres: pshift without the flag (everything the flag does for a code-0 group, and everything code 6 does behind the sum)
struct ShapeSpec {
    int base = 0, line_shape = SH_VOIGT;
    bool pshift = false, ped = false, vvh = false;
    bool flag = false;   // CS_SHAPE_PSHIFT was ORed on (pshift without it: code 7)
    // Voigt, Lorentz, pedestal-removed Voigt, Van Vleck-Huber Voigt, both, both shifted: what line_sum_voigt runs.  Its far wings can be
    // interpolated, and gases of a column with the same code and cut-off can share one merged table
    bool voigt_family() const
    {
        return base == SH_VOIGT || base == SH_LORENTZ || base == SH_VOIGT_CKD || base == SH_VOIGT_VVH || base == SH_VOIGT_CKD_VVH || base == SH_VOIGT_LBL;
    }
};
static ShapeSpec shape_spec(int code)   // (of any integer: decode_shape says which ones are shape codes)
{
    ShapeSpec sh;
    sh.flag = code >= 0 && (code & CS_SHAPE_PSHIFT) != 0;
    sh.base = sh.flag ? (code & ~CS_SHAPE_PSHIFT) : code;
    sh.pshift = sh.flag || sh.base == SH_VOIGT_LBL;
    sh.ped = sh.base == SH_VOIGT_CKD || sh.base == SH_VOIGT_CKD_VVH || sh.base == SH_VOIGT_LBL;
    sh.vvh = sh.base == SH_VOIGT_VVH || sh.base == SH_VOIGT_CKD_VVH || sh.base == SH_VOIGT_LBL;
    sh.line_shape = (sh.ped || sh.vvh) ? SH_VOIGT : sh.base;
    return sh;
}
// ... any other bit, and the flag on another code (code 7 included: it needs none and accepts none), is refused
static int decode_shape(int code, ShapeSpec &sh)
{
    sh = shape_spec(code);
    if (sh.base < 0 || sh.base > SH_VOIGT_LBL) return fail(CS_EINVAL, "unknown shape %d", code);
    if (sh.flag && sh.base > SH_DOPPLER) return fail(CS_EINVAL, "CS_SHAPE_PSHIFT applies to shape codes 0, 1 and 2, not to %d", sh.base);
    return CS_OK;
}
// the largest pressure shift a line of G can take at pressures P[0..n): max |delta_a| x max P / P0 (every decision made from table positions
// is widened by it).  A flagged or code-7 group on a table without shifts is an error, not a shift of zero.
static int shift_width(const GasTable &G, const double *P, int64_t n, double &ds)
{
    if (G.h_da.empty()) return fail(CS_EINVAL, "CS_SHAPE_PSHIFT or CS_SHAPE_VOIGT_LBL on a gas without pressure shifts (load its table with cs_gas_upload_par)");
    double pmax = 0.0;
    for (int64_t k = 0; k < n; k++) pmax = std::max(pmax, std::fabs(P[k]));
    ds = G.da_max * pmax / kAtm * (1.0 + 1e-12);
    return CS_OK;
}

int check_gas_states(const GasTable &G, int K, const double *T)
{
    for (int k = 0; k < K; k++)
        if (!(T[k] >= kTmin && T[k] <= kTmax))
            return fail(CS_ETEMP, "temperature %g K outside of Qref/Q interpolation range [25, 1000]", T[k]);
    for (int64_t j = 0; j < G.L; j++) {
        int I = G.h_iso[j];
        if (I < 1 || I > G.niso || G.h_ncheb[I - 1] <= 0)
            return fail(CS_ENOCHEB, "no interpolating polynomial available to compute Qref/Q for isotopologue %d", I);
    }
    return CS_OK;
}

int check_ascending(const double *nu, int64_t n)
{
    if (n < 1) return fail(CS_EINVAL, "empty wavenumber vector");
    for (int64_t i = 1; i < n; i++)
        if (!(nu[i] > nu[i - 1])) return fail(CS_EORDER, "wavenumber vectors must be sorted in ascending order");
    return CS_OK;
}

}  // namespace

extern "C" {

int cs_version(void) { return 100; }
#ifndef CS_BUILD_ID
#define CS_BUILD_ID "unknown"
#endif
const char *cs_build_id(void) { return CS_BUILD_ID; }
const char *cs_last_error(void) { return g_err.c_str(); }

int cs_create(int device, cs_ctx **out)
{
    if (!out) return fail(CS_EINVAL, "out is NULL");
    int n = 0;
    HIPCHK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(CS_EINVAL, "device %d out of range (%d devices)", device, n);
    HIPCHK(hipSetDevice(device));
    cs_ctx *c = new cs_ctx();
    c->device = device;
    {   // the code object is built for gfx950 only; k_flux_*'s in-kernel band sum (flux_last_block_reduce) additionally relies on a
        // property of that architecture -- see its comment -- so it is switched on by the device's name, not assumed
        hipDeviceProp_t prop;
        c->gfx950 = hipGetDeviceProperties(&prop, device) == hipSuccess && strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork3, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join3, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_far3, hipEventDisableTiming);
    if (e != hipSuccess) { cs_destroy(c); return fail(CS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    {   // R_n[m][j] = l_j(x_m): Lagrange basis of the n extrema cos(pi j / (n - 1)) at the 64 extrema cos(pi m / 63), barycentric form
        std::vector<double> R((size_t)CS_NC * 48);
        const long double pi = 3.14159265358979323846264338327950288L;
        for (int n : {32, 16}) {
            double *Rn = R.data() + (n == 32 ? 0 : CS_NC * 32);
            std::vector<long double> x(n), w(n);
            for (int j = 0; j < n; j++) { x[j] = cosl(pi * j / (n - 1)); w[j] = ((j & 1) ? -1.0L : 1.0L) * ((j == 0 || j == n - 1) ? 0.5L : 1.0L); }
            for (int m = 0; m < CS_NC; m++) {
                const long double xm = cosl(pi * m / (CS_NC - 1));
                int hit = -1;
                long double den = 0.0L;
                for (int j = 0; j < n; j++) {
                    const long double d = xm - x[j];
                    if (fabsl(d) < 1e-17L) hit = j; else den += w[j] / d;
                }
                for (int j = 0; j < n; j++)
                    Rn[(size_t)m * n + j] = hit >= 0 ? (j == hit ? 1.0 : 0.0) : (double)((w[j] / (xm - x[j])) / den);
            }
        }
        if (upload(c->reinterp, R.data(), R.size(), c->stream) != CS_OK || hipStreamSynchronize(c->stream) != hipSuccess) {
            cs_destroy(c);
            return fail(CS_EHIP, "upload of the re-interpolation matrices failed");
        }
    }
    *out = c;
    c->counted = true;
    g_live_ctx++;
    return CS_OK;
}

void cs_destroy(cs_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->counted && --g_live_ctx == 0) pool_stop();
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    drop_graph(ctx->col);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->ev_fork3) (void)hipEventDestroy(ctx->ev_fork3);
    if (ctx->ev_join3) (void)hipEventDestroy(ctx->ev_join3);
    if (ctx->ev_far3) (void)hipEventDestroy(ctx->ev_far3);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// host mirror -> statistics + device arrays
static int table_to_device(GasTable &G, hipStream_t s)
{
    const int64_t L = G.L;
    G.mu_min = *std::min_element(G.h_mu.begin(), G.h_mu.end());
    G.mu_max = *std::max_element(G.h_mu.begin(), G.h_mu.end());
    G.ga_max = *std::max_element(G.h_ga.begin(), G.h_ga.end());
    G.gs_max = *std::max_element(G.h_gs.begin(), G.h_gs.end());
    G.na_min = *std::min_element(G.h_na.begin(), G.h_na.end());
    G.na_max = *std::max_element(G.h_na.begin(), G.h_na.end());
    if (!(G.mu_min > 0)) return fail(CS_EINVAL, "isotopologue molar masses must be positive");
    std::vector<double> sref(L);   // scaleintensity, line_shapes.jl:107-123: the denominator at Tref does not depend on the state
    for (int64_t j = 0; j < L; j++) sref[j] = G.h_S[j] / (std::exp(-kC2 * G.h_Epp[j] / kTref) * (1.0 - std::exp(-kC2 * G.h_nu[j] / kTref)));
    int rc;
    if ((rc = upload(G.sref, sref.data(), L, s))) return rc;
    if ((rc = upload(G.nu, G.h_nu.data(), L, s)) || (rc = upload(G.S, G.h_S.data(), L, s)) || (rc = upload(G.ga, G.h_ga.data(), L, s)) ||
        (rc = upload(G.gs, G.h_gs.data(), L, s)) || (rc = upload(G.Epp, G.h_Epp.data(), L, s)) || (rc = upload(G.na, G.h_na.data(), L, s)) ||
        (rc = upload(G.mu, G.h_mu.data(), L, s)) || (rc = upload(G.iso, G.h_iso.data(), L, s)) || (rc = upload(G.ncheb, G.h_ncheb.data(), G.niso, s)) ||
        (rc = upload(G.cheb, G.h_cheb.data(), (size_t)G.niso * CS_CHEB_LD, s)))
        return rc;
    if (!G.h_gid.empty() && (rc = upload(G.gid, G.h_gid.data(), L, s))) return rc;
    G.da_max = 0.0;
    for (double d : G.h_da) G.da_max = std::max(G.da_max, std::fabs(d));
    HIPCHK(hipStreamSynchronize(s));   // (sref is a local)
    G.present = true;
    return CS_OK;
}

static uint64_t next_generation()   // (cs_fluxes_discretized_multi sets columns up on one host thread per context)
{
    static std::atomic<uint64_t> g{0};
    return ++g;
}

int cs_gas_upload(cs_ctx *ctx, int slot, int64_t L, const double *nu, const double *S, const double *gamma_a,
                  const double *gamma_s, const double *Epp, const double *na, const double *mu_iso,
                  const int16_t *iso, int niso, const int32_t *ncheb, const double *cheb)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (slot < 0 || slot >= CS_MAX_GAS) return fail(CS_EINVAL, "gas slot %d out of range", slot);
    if (L < 1 || niso < 1) return fail(CS_EINVAL, "empty line table");
    for (int64_t j = 1; j < L; j++)
        if (!(nu[j] >= nu[j - 1])) return fail(CS_EORDER, "line table must be sorted by wavenumber (par.jl:267)");
    // line indices travel as int32 (windows, zones) and as 26-bit fields of the near-line queue entries (k_voigt_near)
    if (L >= ((int64_t)1 << kNearLineBits)) return fail(CS_EINVAL, "line table too long (%lld lines; the limit is 2^26 - 1 per gas)", (long long)L);
    HIPCHK(hipSetDevice(ctx->device));
    GasTable &G = ctx->gas[slot];
    G.present = false;
    G.L = L;
    G.niso = niso;
    G.h_nu.assign(nu, nu + L); G.h_S.assign(S, S + L); G.h_ga.assign(gamma_a, gamma_a + L); G.h_gs.assign(gamma_s, gamma_s + L);
    G.h_Epp.assign(Epp, Epp + L); G.h_na.assign(na, na + L); G.h_mu.assign(mu_iso, mu_iso + L);
    G.h_iso.assign(iso, iso + L);
    G.h_ncheb.assign(ncheb, ncheb + niso);
    G.h_cheb.assign(cheb, cheb + (size_t)niso * CS_CHEB_LD);
    G.h_gid.clear();
    G.members.clear();
    G.h_da.clear();   // (a new table drops the shifts of the old one)
    G.da.release();
    int rc;
    if ((rc = table_to_device(G, ctx->stream))) return rc;
    G.generation = next_generation();
    return CS_OK;
}

// HITRAN's air pressure shifts delta_a [cm^-1/atm] of the table just uploaded into `slot`, line for line (CS_SHAPE_PSHIFT): kept on the host
// with the table (cs_gas_upload_par); the device copy is made at the first flagged use (ensure_shifts), so unflagged use costs nothing
static int attach_shift(cs_ctx *ctx, int slot, int64_t L, const double *delta_a)
{
    GasTable &G = ctx->gas[slot];
    if (L != G.L) return fail(CS_EINVAL, "%lld pressure shifts for a table of %lld lines", (long long)L, (long long)G.L);
    for (int64_t j = 0; j < L; j++)
        if (!std::isfinite(delta_a[j])) return fail(CS_EINVAL, "pressure shift of line %lld is not finite", (long long)j);
    G.h_da.assign(delta_a, delta_a + L);
    G.da_max = 0.0;
    for (double d : G.h_da) G.da_max = std::max(G.da_max, std::fabs(d));
    return CS_OK;
}

// the device copy of a table's shifts, made once (the caller has checked that there are shifts: shift_width)
static int ensure_shifts(const GasTable &G, hipStream_t s)
{
    if (G.da.p) return CS_OK;
    int rc;
    if ((rc = upload(G.da, G.h_da.data(), (size_t)G.L, s))) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return CS_OK;
}

// One sorted table out of the tables of `slots` (stable merge by wavenumber: lines of equal position keep member order), each
// line tagged with its member index; isotopologue numbers are offset into the concatenated Chebyshev tables.  Kept by the context
// (a handful, keyed by the members' upload generations) so that re-setting a column up does not merge again.
static int merged_table(cs_ctx *ctx, const std::vector<int> &slots, std::shared_ptr<const GasTable> *out)
{
    std::vector<std::pair<int, uint64_t>> key;
    for (int sl : slots) key.emplace_back(sl, ctx->gas[sl].generation);
    for (size_t i = 0; i < ctx->merged.size(); i++)
        if (ctx->merged[i]->members == key) {   // a hit becomes the most recently used entry
            std::shared_ptr<GasTable> m = ctx->merged[i];
            ctx->merged.erase(ctx->merged.begin() + i);
            ctx->merged.push_back(m);
            *out = m;
            return CS_OK;
        }
    // the cache only bounds what the CONTEXT keeps: a column shares ownership of the tables of its launch groups (ColGas::hold), so
    // evicting the least recently used entry can never free a table a column still runs on, however many groups that column has
    if (ctx->merged.size() >= CS_MAX_GAS / 2) ctx->merged.erase(ctx->merged.begin());
    int64_t L = 0;
    int niso = 0;
    for (int sl : slots) { L += ctx->gas[sl].L; niso += ctx->gas[sl].niso; }
    if (L >= ((int64_t)1 << kNearLineBits)) return fail(CS_EINVAL, "merged line table too long (%lld lines; the limit is 2^26 - 1)", (long long)L);
    std::shared_ptr<GasTable> M(new GasTable());
    GasTable &G = *M;
    G.L = L;
    G.niso = niso;
    G.members = key;
    struct Src { uint8_t m; int32_t j; };
    std::vector<Src> order, next, mine;
    std::vector<int> iso_off(slots.size());
    int off = 0;
    auto nu_of = [&](const Src &q) { return ctx->gas[slots[q.m]].h_nu[q.j]; };
    for (size_t m = 0; m < slots.size(); m++) {   // members are sorted: merge them one by one (stable: equal positions keep member order)
        const GasTable &g = ctx->gas[slots[m]];
        iso_off[m] = off;
        off += g.niso;
        mine.resize((size_t)g.L);
        for (int64_t j = 0; j < g.L; j++) mine[j] = Src{(uint8_t)m, (int32_t)j};
        next.resize(order.size() + mine.size());
        std::merge(order.begin(), order.end(), mine.begin(), mine.end(), next.begin(), [&](const Src &a, const Src &b) { return nu_of(a) < nu_of(b); });
        order.swap(next);
        G.h_ncheb.insert(G.h_ncheb.end(), g.h_ncheb.begin(), g.h_ncheb.end());
        G.h_cheb.insert(G.h_cheb.end(), g.h_cheb.begin(), g.h_cheb.end());
    }
    G.h_nu.resize(L); G.h_S.resize(L); G.h_ga.resize(L); G.h_gs.resize(L); G.h_Epp.resize(L); G.h_na.resize(L); G.h_mu.resize(L);
    G.h_iso.resize(L); G.h_gid.resize(L);
    bool all_da = true;
    for (int sl : slots) all_da = all_da && !ctx->gas[sl].h_da.empty();
    if (all_da) G.h_da.resize(L);   // (shifts only where every member has them: a flagged group refuses a table without)
    for (int64_t i = 0; i < L; i++) {
        const Src q = order[i];
        const GasTable &g = ctx->gas[slots[q.m]];
        G.h_nu[i] = g.h_nu[q.j]; G.h_S[i] = g.h_S[q.j]; G.h_ga[i] = g.h_ga[q.j]; G.h_gs[i] = g.h_gs[q.j];
        G.h_Epp[i] = g.h_Epp[q.j]; G.h_na[i] = g.h_na[q.j]; G.h_mu[i] = g.h_mu[q.j];
        G.h_iso[i] = (int16_t)(g.h_iso[q.j] + iso_off[q.m]);
        G.h_gid[i] = q.m;
        if (all_da) G.h_da[i] = g.h_da[q.j];
    }
    int rc;
    if ((rc = table_to_device(G, ctx->stream))) return rc;
    G.generation = next_generation();
    *out = M;
    ctx->merged.push_back(std::move(M));
    return CS_OK;
}

int cs_set_precision(cs_ctx *ctx, int mode, double far_s)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (mode != 0 && mode != 1) return fail(CS_EINVAL, "precision mode must be 0 (fp64) or 1 (fp32 far wings)");
    if (!(far_s >= 1e6)) return fail(CS_EINVAL, "far_s must be >= 1e6");
    ctx->mixed = mode;
    ctx->far_s = far_s;
    drop_graph(ctx->col);
    return CS_OK;
}

int cs_set_interp(cs_ctx *ctx, int on)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    ctx->interp = on ? 1 : 0;
    return CS_OK;
}

int cs_set_interp_plan(cs_ctx *ctx, int first_level, int size_min, int size_max)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (size_min < 128 || size_max > 2048 || size_min > size_max) return fail(CS_EINVAL, "interval sizes must satisfy 128 <= size_min <= size_max <= 2048");
    if (first_level < -1 || first_level > CS_MAX_LEVEL) return fail(CS_EINVAL, "first_level must be -1 (automatic) or 0..%d", CS_MAX_LEVEL);
    ctx->itp_first = first_level;
    ctx->itp_min = size_min;
    ctx->itp_max = size_max;
    return CS_OK;
}

int cs_set_matrix_cores(cs_ctx *ctx, int on)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (on < 0) on = 0;
    set_matrix_cores(ctx->set, on);
    drop_graph(ctx->col);
    return CS_OK;
}

int cs_set_merge(cs_ctx *ctx, int on)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    ctx->merge = on ? 1 : 0;
    return CS_OK;
}

static int interp_key(const cs_ctx *ctx)
{
    return (ctx->set.rt_streams ? 65536 : 0) + ctx->interp * 4096 + (ctx->itp_first + 1) * 256 + (ctx->itp_min >> 7) * 16 + (ctx->itp_max >> 7);
}

constexpr int CS_NTUNE = 24;   // keys 0 .. 23 are accepted
int cs_set_tuning(cs_ctx *ctx, int key, int value)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (key < 0 || key >= CS_NTUNE) return fail(CS_EINVAL, "tuning key %d out of range", key);
    if (key == CS_TUNE_MARGIN && value != 0 && (value < 15 || value > 100)) return fail(CS_EINVAL, "interpolation margin must be 15..100 per cent of the half-width");
    if (key == CS_TUNE_SUB_LEAN && (value < 0 || value > 2)) return fail(CS_EINVAL, "range-only pass of k_voigt_sub: 0 (by the tables), 1 (never) or 2 (always first)");
    set_tuning(ctx->set, key, value);
    drop_graph(ctx->col);
    return CS_OK;
}

int cs_gas_clear(cs_ctx *ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= CS_MAX_GAS) return fail(CS_EINVAL, "bad slot");
    for (auto &g : ctx->col.ugas)
        if (g.slot == slot) ctx->col.ready = false;   // (the resident column's windows belong to the table that goes away)
    ctx->gas[slot] = GasTable();
    return CS_OK;
}

// The windows of a launch group of table G on the grid nu: the included lines (strict: the end-point pre-filter of the vector method, else every
// line), the windows of the 256- and 64-point tiles, the record range they span, the far kernel's block order -- all widened by ds, the group's
// largest shift (the caller's, from shift_width, after check_near_density passed with it).  Uploaded when it returns.
static int build_windows(GroupWindows &w, const GasTable &G, const ShapeSpec &sh, double cut, double ds, const double *nu, int64_t nnu, bool strict,
                         hipStream_t s)
{
    int rc;
    w.ds = ds;
    if (sh.pshift && (rc = ensure_shifts(G, s))) return rc;
    included_range(G.h_nu, nu[0], nu[nnu - 1], cut + ds, strict, w.g0, w.g1);
    std::vector<int32_t> J0, J1;
    tile_windows(G.h_nu, w.g0, w.g1, nu, nnu, window_reach(sh.line_shape, G, nu[nnu - 1] + ds, cut) + ds, J0, J1);
    w.ntile256 = (int)J0.size();
    w.jlo = J0.front();
    w.jhi = J1.back();
    w.pa = std::max(w.g0, w.jlo);
    w.pb = std::min(w.g1, w.jhi);
    w.mb = sh.vvh ? vvh_mirror_end(G.h_nu, w.pa, w.pb, nu[0], cut, ds) : w.pa;
    std::vector<WaveWin> win;
    w.xtiles = wave_windows(G.h_nu, w.g0, w.g1, nu, nnu, cut, win, 64, ds);
    w.nwin = (int)win.size();
    if ((rc = upload(w.J0, J0.data(), J0.size(), s)) || (rc = upload(w.J1, J1.data(), J1.size(), s)) || (rc = upload(w.win, win.data(), win.size(), s)))
        return rc;
    HIPCHK(hipStreamSynchronize(s));   // J0, J1, win are locals
    return CS_OK;
}

static void pass_windows(GasPass &p, const GroupWindows &w)
{
    p.jlo = w.jlo; p.jhi = w.jhi; p.pa = w.pa; p.pb = w.pb; p.mb = w.mb; p.ds = w.ds;
    p.ntile256 = w.ntile256; p.J0 = w.J0.as<int32_t>(); p.J1 = w.J1.as<int32_t>(); p.win = w.win.as<WaveWin>(); p.xtiles = w.xtiles;
}

// element idx of every state's row of conc [N][stride] -- a column's gases, or its tables, at its node states; B columns one after the
// other are B K such rows -- checked and gathered into out[N]
static int gather_conc(const double *conc, int idx, int stride, int64_t N, double *out)
{
    for (int64_t n = 0; n < N; n++) {
        out[n] = conc[idx + (size_t)stride * n];
        if (!(out[n] >= 0 && out[n] <= 1)) return fail(CS_EINVAL, "gas molar concentrations must be in [0,1], not %g", out[n]);
    }
    return CS_OK;
}

// What a group of table G needs per state, at N states (T, P): from the partial pressures pp [nmem][N] of its members (tables mem[nmem]; a
// gas on its own is its one member) the Lorentz-width bound over the members, and the state tables of G; Pp, gmax, lrt, qref uploaded
static int upload_group_states(hipStream_t s, GroupStates &st, const GasTable &G, const GasTable *const *mem, int nmem, int64_t N, const double *T,
                               const double *P, const double *pp)
{
    std::vector<double> gb, lrt, qr;
    for (int m = 0; m < nmem; m++) {
        const std::vector<double> gm = gamma_bound(*mem[m], (int)N, T, P, pp + (size_t)m * N);
        if (m == 0) gb = gm;
        else
            for (int64_t k = 0; k < N; k++) gb[k] = std::max(gb[k], gm[k]);
    }
    state_tables(G, (int)N, T, lrt, qr);
    st.h_T.assign(T, T + N);
    st.h_gmax = gb;
    int rc;
    if ((rc = upload(st.Pp, pp, (size_t)nmem * N, s)) || (rc = upload(st.gmax, gb.data(), N, s)) || (rc = upload(st.lrt, lrt.data(), lrt.size(), s)) ||
        (rc = upload(st.qref, qr.data(), qr.size(), s)))
        return rc;
    HIPCHK(hipStreamSynchronize(s));   // (locals)
    return CS_OK;
}

// ... of a launch group of the resident column, at N of its node states (one set of them, or a batch's B sets one after the other) with the
// concentrations conc [N][ngas] of the column's gases: Pp = C P of every member (gases.jl:126), and the members' concentrations themselves
static int column_group_states(cs_ctx *ctx, const ColGas &cg, GroupStates &st, int64_t N, const double *T, const double *P, const double *conc,
                               hipStream_t s)
{
    const Column &c = ctx->col;
    const int nm = (int)cg.mem.size();
    std::vector<double> cc((size_t)nm * N), pp((size_t)nm * N);
    std::vector<const GasTable *> mem(nm);
    int rc;
    for (int m = 0; m < nm; m++) {
        if ((rc = gather_conc(conc, cg.mem[m], c.ngas, N, cc.data() + (size_t)m * N))) return rc;
        for (int64_t n = 0; n < N; n++) pp[(size_t)m * N + n] = cc[(size_t)m * N + n] * P[n];
        mem[m] = &ctx->gas[c.ugas[cg.mem[m]].slot];
    }
    if ((rc = upload(st.conc, cc.data(), cc.size(), s))) return rc;
    return upload_group_states(s, st, *cg.tab, mem.data(), nm, N, T, P, pp.data());
}

static void pass_states(GasPass &p, const GroupStates &st, int64_t k0)   // states k0 .. of st (p.G is set; p.scale is the caller's: only columns have one)
{
    p.Ppk = st.Pp.as<double>() + k0; p.gbound = st.gmax.as<double>() + k0;
    p.h_Tk = st.h_T.data() + k0; p.h_gbound = st.h_gmax.data() + k0;
    p.lrt = st.lrt.as<double>() + k0; p.qrefq = st.qref.as<double>() + (size_t)k0 * p.G->niso;
}

// the line workspace of kn states of tables of at most maxL lines on nnu points: the records, and where asked for (NULL: not) the near-line
// ranges with the per-(tile, state) flags, the fp32 records of mixed precision, launch_pedestal's workspace, the spare plane of a second code-5/6 group
static int reserve_lines(size_t kn, size_t maxL, int64_t nnu, DevBuf &hot, DevBuf &cold, DevBuf *ranges, DevBuf *hot32, DevBuf *ped, DevBuf *spare)
{
    HIPCHK(hot.reserve((kn * maxL + 4) * sizeof(LineHot)));
    HIPCHK(cold.reserve(kn * maxL * sizeof(LineCold)));
    if (ranges) HIPCHK(ranges->reserve(NearHandoff<unsigned>::bytes(kn, nnu)));
    if (hot32) HIPCHK(hot32->reserve((kn * maxL + 4) * sizeof(LineF32)));
    if (ped) HIPCHK(ped->reserve(ped_bytes((int64_t)kn, (int64_t)maxL)));
    if (spare) HIPCHK(spare->reserve(kn * nnu * sizeof(double)));
    return CS_OK;
}

// where gas_states puts sigma [K][nnu]: host rows of pitch ld (it owns the buffer of a chunk and copies each chunk out), or a device plane
// written in place, which plane() hands out once the call has passed its checks (cs_bake: only then is the table in the slot given up)
struct StatesOut {
    double *host = nullptr;
    int64_t ld = 0;
    std::function<int(double *&)> plane;
};

// sigma of one gas at K states on the grid nu, behind cs_shape_batch / cs_shape_points / cs_bake (which have checked the slot, the shape
// code, their sizes and the grid): the states in chunks that bound the workspace
static int gas_states(cs_ctx *ctx, GasTable &G, const ShapeSpec &sh, double dnu_cut, int64_t nnu, const double *nu, int K,
                      const double *T, const double *P, const double *Pp, bool strict, const StatesOut &out)
{
    int rc;
    const int shape = sh.line_shape;
    const bool ped = sh.ped;
    double ds = 0.0;   // CS_SHAPE_PSHIFT: every window and the line range widened by the largest shift of these states
    if (sh.pshift && (rc = shift_width(G, P, K, ds))) return rc;
    if ((rc = check_gas_states(G, K, T))) return rc;
    if (shape == SH_VOIGT && (rc = check_near_density(G, nu, nnu, dnu_cut, ds))) return rc;
    ph_set_grid(ctx, nu, nnu, ++g_grid_counter);
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    double *Z = nullptr;   // the caller's plane; NULL: a chunk buffer of our own, copied to out.host
    if (out.plane && (rc = out.plane(Z))) return rc;
    GroupWindows w;
    GroupStates st;        // (one member, the caller's Pp: no concentration plane)
    const GasTable *mem = &G;
    if ((rc = build_windows(w, G, sh, dnu_cut, ds, nu, nnu, strict, s)) || (rc = upload_group_states(s, st, G, &mem, 1, K, T, P, Pp))) return rc;
    DevBuf dnu, dT, dP, hot, cold, hot32, dsig, dzones, dranges, dped;
    if ((rc = upload(dnu, nu, nnu, s)) || (rc = upload(dT, T, K, s)) || (rc = upload(dP, P, K, s))) return rc;
    // bound the workspace: process the states in chunks
    const size_t per_state = (size_t)G.L * (sizeof(LineHot) + sizeof(LineCold)) +
                             (Z ? (size_t)nnu * kNearPointBytes : (size_t)nnu * (sizeof(double) + kNearPointBytes)) + (ped ? ped_bytes(1, G.L) : 0);
    const int kc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)K, ((size_t)4 << 30) / per_state, (size_t)65535}));   // gridDim.y limit
    const bool mixed = ctx->mixed && shape == SH_VOIGT && !sh.pshift;
    if ((rc = reserve_lines(kc, G.L, nnu, hot, cold, &dranges, mixed ? &hot32 : nullptr, ped ? &dped : nullptr, nullptr))) return rc;
    if (!Z) HIPCHK(dsig.reserve((size_t)kc * nnu * sizeof(double)));
    HIPCHK(dzones.reserve((size_t)kc * w.nwin * sizeof(Zone)));
    GasPass p;
    p.G = &G; p.shape = shape; p.cut = dnu_cut; p.ped = ped; p.vvh = sh.vvh;
    pass_windows(p, w);
    // (the strict pre-filter of a shifted line is its own state's: prep_body parks the lines whose shifted centre fails it)
    p.pshift = sh.pshift; p.flo = strict ? nu[0] - dnu_cut : -INFINITY; p.fhi = strict ? nu[nnu - 1] + dnu_cut : INFINITY;
    p.dnu = dnu.as<double>(); p.nu = nu; p.nnu = nnu;
    p.hot = hot.as<LineHot>(); p.cold = cold.as<LineCold>(); p.zones = dzones.as<Zone>(); p.ranges = dranges.as<unsigned>(); p.ped_ws = dped.as<double>();
    if (mixed) p.hot32 = hot32.as<LineF32>();
    p.clamp = true;   // the gas's own sigma, complete
    p.far_s = ctx->far_s; p.ph = &ctx->ph;
    ChebGrid cheb;
    GasInterp ginterp;
    if (ctx->interp && sh.voigt_family()) {
        if ((rc = cheb_build(ctx, cheb, nu, dnu.as<double>(), nnu, dnu_cut, s)) ||
            (rc = gas_interp_build(ctx, ginterp, cheb, G.h_nu, w.g0, w.g1, nu, nnu, dnu_cut, kc, s, true, w.ds)))
            return rc;
        p.itp = interp_view(cheb, ginterp, kc);
        interp_select(ctx, p.itp);
        p.set = &ctx->set;
    }
    for (int k0 = 0; k0 < K; k0 += kc) {
        p.kn = std::min(kc, K - k0);
        p.Tk = dT.as<double>() + k0; p.Pk = dP.as<double>() + k0;
        pass_states(p, st, k0);
        p.sigma = Z ? Z + (size_t)k0 * nnu : dsig.as<double>();
        launch_gas(s, p);
        HIPCHK(hipGetLastError());
        if (!Z)
            HIPCHK(hipMemcpy2DAsync(out.host + (size_t)k0 * out.ld, out.ld * sizeof(double), dsig.p, nnu * sizeof(double), nnu * sizeof(double), p.kn,
                                    hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
    }
    return CS_OK;
}

static int shape_impl(cs_ctx *ctx, int slot, int shape, double dnu_cut, int64_t nnu, const double *nu, int K,
                      const double *T, const double *P, const double *Pp, double *sigma, int64_t ld_state, bool strict)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (slot < 0 || slot >= CS_MAX_GAS || !ctx->gas[slot].present) return fail(CS_EINVAL, "gas slot %d is empty", slot);
    ShapeSpec sh;
    int rc;
    if ((rc = decode_shape(shape, sh))) return rc;
    if (K < 1 || ld_state < nnu) return fail(CS_EINVAL, "bad K/ld_state");
    if ((rc = check_ascending(nu, nnu))) return rc;
    StatesOut out;
    out.host = sigma; out.ld = ld_state;   // no plane: gas_states owns the chunk buffer
    return gas_states(ctx, ctx->gas[slot], sh, dnu_cut, nnu, nu, K, T, P, Pp, strict, out);
}

int cs_shape_batch(cs_ctx *ctx, int slot, int shape, double dnu_cut, int64_t nnu, const double *nu, int K,
                   const double *T, const double *P, const double *Pp, double *sigma, int64_t ld_state)
{
    return shape_impl(ctx, slot, shape, dnu_cut, nnu, nu, K, T, P, Pp, sigma, ld_state, true);
}

int cs_shape_points(cs_ctx *ctx, int slot, int shape, double dnu_cut, int64_t nnu, const double *nu, int K,
                    const double *T, const double *P, const double *Pp, double *sigma, int64_t ld_state)
{
    return shape_impl(ctx, slot, shape, dnu_cut, nnu, nu, K, T, P, Pp, sigma, ld_state, false);
}

int cs_bake(cs_ctx *ctx, int gas_slot, int table_slot, int shape, double dnu_cut, int64_t nnu, const double *nu, int nT,
            const double *T, int nP, const double *P, const double *conc, double *lnsigma_out)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (gas_slot < 0 || gas_slot >= CS_MAX_GAS || !ctx->gas[gas_slot].present) return fail(CS_EINVAL, "gas slot %d is empty", gas_slot);
    if (table_slot < 0 || table_slot >= CS_MAX_TABLE) return fail(CS_EINVAL, "table slot %d out of range", table_slot);
    ShapeSpec sh;
    int rc;
    if ((rc = decode_shape(shape, sh))) return rc;
    if (nT < 2 || nP < 2) return fail(CS_EINVAL, "need at least 2 x 2 grid points");
    if ((rc = check_ascending(nu, nnu))) return rc;
    for (int64_t i = 0; i < nnu; i++)
        if (!(nu[i] >= 0)) return fail(CS_EINVAL, "wavenumbers must be positive");
    const int M = nT * nP;
    std::vector<double> Ts(M), Ps(M), Pp(M);
    for (int j = 0; j < nP; j++)
        for (int i = 0; i < nT; i++) {
            const double C = conc[i + (size_t)nT * j];
            if (!(C >= 0 && C <= 1)) return fail(CS_EINVAL, "gas molar concentrations must be in [0,1], not %g (encountered @ %g K, %g Pa)", C, T[i], P[j]);
            Ts[i + nT * j] = T[i];
            Ps[i + nT * j] = P[j];
            Pp[i + nT * j] = C * P[j];
        }
    TableDev &tb = ctx->tab[table_slot];
    StatesOut out;   // straight into the table's Z; a call refused before this leaves a table already in the slot usable
    out.plane = [&](double *&Z) {
        tb.present = false;
        HIPCHK(tb.Z.reserve((size_t)M * nnu * sizeof(double)));
        Z = tb.Z.as<double>();
        return (int)CS_OK;
    };
    // (bake uses the vector method: strict pre-filter, per state when shifted; codes 4, 6 clamped before k_table_log)
    if ((rc = gas_states(ctx, ctx->gas[gas_slot], sh, dnu_cut, nnu, nu, M, Ts.data(), Ps.data(), Pp.data(), true, out))) return rc;
    hipStream_t s = ctx->stream;
    CS_LAUNCH(k_table_log, dim3((unsigned)((nnu + 255) / 256)), dim3(256), 0, s, tb.Z.as<double>(), M, nnu);
    HIPCHK(hipGetLastError());
    if (lnsigma_out) HIPCHK(hipMemcpyAsync(lnsigma_out, tb.Z.p, (size_t)M * nnu * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    tb.nnu = nnu; tb.nT = nT; tb.nP = nP;
    tb.T.assign(T, T + nT);
    tb.lnP.resize(nP);
    for (int j = 0; j < nP; j++) tb.lnP[j] = std::log(P[j]);
    tb.nu.assign(nu, nu + nnu);
    tb.generation = next_generation();
    tb.present = true;
    return CS_OK;
}

int cs_table_clear(cs_ctx *ctx, int table_slot)
{
    if (!ctx || table_slot < 0 || table_slot >= CS_MAX_TABLE) return fail(CS_EINVAL, "bad table slot");
    ctx->tab[table_slot] = TableDev();
    return CS_OK;
}

// sigma[k][nu] += conc[k] * exp(sum_m Z[m][nu] W[m][k]) for K states (the Gas functor, gases.jl:85,278)
#ifndef CS_TABLE_NSUB
#define CS_TABLE_NSUB 2
#endif
static int launch_table_eval(hipStream_t s, const TableDev &tb, const TabStates &st, int K, double *sigma)
{
    const int nt64 = (int)((tb.nnu + 63) / 64);
    const int nst = (K + 15) / 16, nsg = (nst + CS_TABLE_NSUB - 1) / CS_TABLE_NSUB;
    const int64_t nblk = (int64_t)((nt64 + 3) / 4) * nsg;
    if (nblk > 0x7fffffffLL) return fail(CS_EINVAL, "too many (tile, state) blocks for the opacity-table kernel");
    CS_LAUNCH(k_table_eval_mfma<CS_TABLE_NSUB>, dim3((unsigned)nblk), dim3(256), 0, s, tb.Z.as<double>(), tb.nT * tb.nP, tb.nnu, nt64,
              st.W.as<double>(), K, st.conc.as<double>(), sigma);
    return CS_OK;
}

// W[m][k] = a_i(T_k) b_j(ln P_k), m = i + nT*j
static int table_weights(const TableDev &tb, int K, const double *Tk, const double *Pk, std::vector<double> &W)
{
    const int M = tb.nT * tb.nP;
    W.assign((size_t)M * K, 0.0);
    std::vector<double> a, b;
    for (int k = 0; k < K; k++) {
        const double lp = std::log(Pk[k]);
        if (!(Tk[k] >= tb.T.front() && Tk[k] <= tb.T.back()))
            return fail(CS_EINVAL, "temperature %g K outside the opacity table's domain [%g, %g]", Tk[k], tb.T.front(), tb.T.back());
        if (!(lp >= tb.lnP.front() - 1e-12 && lp <= tb.lnP.back() + 1e-12))
            return fail(CS_EINVAL, "Pressure %g Pa outside the opacity table's domain [%g, %g]", Pk[k], std::exp(tb.lnP.front()), std::exp(tb.lnP.back()));
        cheb_basis(tb.T, Tk[k], a);
        cheb_basis(tb.lnP, std::min(std::max(lp, tb.lnP.front()), tb.lnP.back()), b);
        for (int j = 0; j < tb.nP; j++)
            for (int i = 0; i < tb.nT; i++) W[(size_t)(i + tb.nT * j) * K + k] = a[i] * b[j];
    }
    return CS_OK;
}

// what table tb needs at N states (T, P): its weights, and element idx of every state's row of conc [N][stride] (NULL: 1 at every state)
static int table_states(hipStream_t s, const TableDev &tb, int64_t N, const double *T, const double *P, const double *conc, int stride, int idx,
                        TabStates &st)
{
    std::vector<double> W, cc(N, 1.0);
    int rc;
    if ((rc = table_weights(tb, (int)N, T, P, W))) return rc;
    if (conc && (rc = gather_conc(conc, idx, stride, N, cc.data()))) return rc;
    if ((rc = upload(st.W, W.data(), W.size(), s))) return rc;
    return upload(st.conc, cc.data(), N, s);   // (from pageable memory: both copies have left the host vectors on return)
}

int cs_table_eval(cs_ctx *ctx, int table_slot, double T, double P, int64_t i0, int64_t n, double *sigma_out)
{
    if (!ctx || table_slot < 0 || table_slot >= CS_MAX_TABLE || !ctx->tab[table_slot].present) return fail(CS_EINVAL, "table slot is empty");
    TableDev &tb = ctx->tab[table_slot];
    if (i0 < 0 || n < 1 || i0 + n > tb.nnu) return fail(CS_EINVAL, "wavenumber range out of bounds");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = table_states(s, tb, 1, &T, &P, nullptr, 0, 0, ctx->tmpTab))) return rc;
    HIPCHK(ctx->tmpC.reserve((size_t)tb.nnu * sizeof(double)));
    HIPCHK(hipMemsetAsync(ctx->tmpC.p, 0, (size_t)tb.nnu * sizeof(double), s));
    if ((rc = launch_table_eval(s, tb, ctx->tmpTab, 1, ctx->tmpC.as<double>()))) return rc;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sigma_out, ctx->tmpC.as<double>() + i0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CS_OK;
}

static int upload_tables(cs_ctx *ctx, const double *conc_tab)
{
    Column &c = ctx->col;
    const int nt = (int)c.tab.size();
    int rc;
    for (int t = 0; t < nt; t++)
        if ((rc = table_states(ctx->stream, ctx->tab[c.tab[t].slot], c.K, c.h_Tk.data(), c.h_Pk.data(), conc_tab, nt, t, c.tab[t].st))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_column_set_tables(cs_ctx *ctx, int ntab, const int *table_slots, const double *conc_tab)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    if (ntab < 0 || ntab > CS_MAX_TABLE) return fail(CS_EINVAL, "ntab out of range");
    Column &c = ctx->col;
    HIPCHK(hipSetDevice(ctx->device));
    drop_graph(c);
    c.tab.clear();
    c.tab.resize(ntab);
    for (int t = 0; t < ntab; t++) {
        const int sl = table_slots[t];
        if (sl < 0 || sl >= CS_MAX_TABLE || !ctx->tab[sl].present) return fail(CS_EINVAL, "table slot %d is empty", sl);
        TableDev &tb = ctx->tab[sl];
        if (tb.nnu != c.nnu || !std::equal(tb.nu.begin(), tb.nu.end(), c.h_nu.begin()))
            return fail(CS_EINVAL, "gases must have identical wavenumber vectors");
        c.tab[t].slot = sl;
        c.tab[t].generation = tb.generation;
    }
    int rc = upload_tables(ctx, conc_tab);
    if (rc) c.tab.clear();
    return rc;
}

int cs_cia_begin(cs_ctx *ctx, int cia_slot, int nband)
{
    if (!ctx || cia_slot < 0 || cia_slot >= CS_MAX_CIA) return fail(CS_EINVAL, "bad CIA slot");
    if (nband < 1 || nband > CS_MAX_CIA_BAND) return fail(CS_EINVAL, "a CIA object holds 1..%d bands", CS_MAX_CIA_BAND);
    ctx->cia[cia_slot] = CiaDev();
    ctx->cia[cia_slot].bands.resize(nband);
    ctx->cia[cia_slot].generation = next_generation();
    return CS_OK;
}

int cs_cia_band(cs_ctx *ctx, int cia_slot, int band, int nb, const double *nu_b, int nt, const double *T_b, const double *lnk)
{
    if (!ctx || cia_slot < 0 || cia_slot >= CS_MAX_CIA) return fail(CS_EINVAL, "bad CIA slot");
    CiaDev &cd = ctx->cia[cia_slot];
    if (band < 0 || band >= (int)cd.bands.size()) return fail(CS_EINVAL, "band index out of range");
    if (nb < 2 || nt < 1) return fail(CS_EINVAL, "a band needs at least 2 wavenumbers and 1 temperature");
    for (int i = 1; i < nb; i++)
        if (!(nu_b[i] > nu_b[i - 1])) return fail(CS_EORDER, "band wavenumbers must be ascending");
    for (int j = 1; j < nt; j++)
        if (!(T_b[j] > T_b[j - 1])) return fail(CS_EORDER, "band temperatures must be ascending");
    HIPCHK(hipSetDevice(ctx->device));
    CiaBandHost &b = cd.bands[band];
    b.nu.assign(nu_b, nu_b + nb);
    b.T.assign(T_b, T_b + nt);
    int rc;
    if ((rc = upload(b.dnu, nu_b, nb, ctx->stream)) || (rc = upload(b.dlnk, lnk, (size_t)nb * nt, ctx->stream))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    cd.filled++;
    cd.present = cd.filled >= (int)cd.bands.size();
    cd.generation = next_generation();
    return CS_OK;
}

int cs_cia_clear(cs_ctx *ctx, int cia_slot)
{
    if (!ctx || cia_slot < 0 || cia_slot >= CS_MAX_CIA) return fail(CS_EINVAL, "bad CIA slot");
    ctx->cia[cia_slot] = CiaDev();
    return CS_OK;
}

// per-state inputs of a CIA pair: temperature cells of every band + number densities (cia(k,T,Pa,P1,P2), :295-303).
// K states with temperatures T, air pressures Pa and partial pressures P1/P2 (element k at P[idx + stride*k]).  An object flagged
// CS_CIA_RADIATION also gets the temperatures themselves (Tr): R(nu, T_k) follows the node states like everything else here
static int cia_states(hipStream_t s, const CiaDev &cd, int flags, int K, const double *T, const double *Pa, const double *P1, const double *P2,
                      int stride, int idx, CiaStates &out)
{
    const int nband = (int)cd.bands.size();
    const bool extrap = flags & CS_CIA_EXTRAPOLATE, singles = flags & CS_CIA_SINGLES;
    std::vector<CiaState> st((size_t)nband * K);
    for (int b = 0; b < nband; b++) {
        const std::vector<double> &Tg = cd.bands[b].T;
        const int nt = (int)Tg.size();
        for (int k = 0; k < K; k++) {
            CiaState q;
            q.use = 0; q.jT = 0; q.fT = 0.0;
            const double Tk = T[k];
            if (nt == 1) {
                q.use = singles ? 1 : 0;
            } else {
                double Te = Tk;
                if (Tk >= Tg.front() && Tk <= Tg.back()) q.use = 1;                       // :258
                else if (extrap) { q.use = 1; Te = Tk > Tg.back() ? Tg.back() : Tg.front(); }  // :261-263
                if (q.use) {
                    int j = (int)(std::upper_bound(Tg.begin(), Tg.end(), Te) - Tg.begin()) - 1;
                    j = std::min(std::max(j, 0), nt - 2);
                    q.jT = j;
                    q.fT = (Te - Tg[j]) / (Tg[j + 1] - Tg[j]);
                }
            }
            st[(size_t)b * K + k] = q;
        }
    }
    std::vector<double> r1(K), r2(K), ra(K);
    for (int k = 0; k < K; k++) {
        r1[k] = (P1[idx + (size_t)stride * k] / kAtm) * (273.15 / T[k]);   // amagat, :297-298 (T0 = 273.15, constants.jl:23)
        r2[k] = (P2[idx + (size_t)stride * k] / kAtm) * (273.15 / T[k]);
        ra[k] = 1e-6 * Pa[k] / (kKb * T[k]);                               // molecules/cm^3, :300
    }
    int rc;
    if ((rc = upload(out.st, st.data(), st.size(), s)) || (rc = upload(out.rho1, r1.data(), K, s)) ||
        (rc = upload(out.rho2, r2.data(), K, s)) || (rc = upload(out.rhoa, ra.data(), K, s)) ||
        ((flags & CS_CIA_RADIATION) && (rc = upload(out.Tr, T, K, s))))
        return rc;
    HIPCHK(hipStreamSynchronize(s));   // the host vectors are locals
    return CS_OK;
}
// k_cia of pair cc over Kn states with the per-state inputs st (the column's own, or a batch's); an object flagged CS_CIA_RADIATION runs k_cia<true>
static void launch_cia(hipStream_t s, const Column &c, const ColCia &cc, const CiaStates &st, int Kn, double *sig)
{
    const CiaGrid &g = cc.grid;
    if (cc.flags & CS_CIA_RADIATION)
        CS_LAUNCH(k_cia<true>, dim3((unsigned)c.ntile), dim3(256), 0, s, g.nband, g.bands.as<CiaBand>(), st.st.as<CiaState>(), c.nu.as<double>(),
                  c.nnu, Kn, st.rho1.as<double>(), st.rho2.as<double>(), st.rhoa.as<double>(), st.Tr.as<double>(), sig);
    else
        CS_LAUNCH(k_cia<false>, dim3((unsigned)c.ntile), dim3(256), 0, s, g.nband, g.bands.as<CiaBand>(), st.st.as<CiaState>(), c.nu.as<double>(),
                  c.nnu, Kn, st.rho1.as<double>(), st.rho2.as<double>(), st.rhoa.as<double>(), (const double *)nullptr, sig);
}
// the pair as the flux kernel and k_cia_tab take it
static CiaPairDev cia_pair(const ColCia &cc)
{
    const CiaGrid &g = cc.grid;
    CiaPairDev pd;
    pd.nband = g.nband; pd.bands = g.bands.as<CiaBand>(); pd.st = cc.st.st.as<CiaState>(); pd.tab = g.tab.as<double>();
    pd.toff = g.toff.as<int64_t>(); pd.rho1 = cc.st.rho1.as<double>(); pd.rho2 = cc.st.rho2.as<double>(); pd.rhoa = cc.st.rhoa.as<double>();
    pd.tband = g.tband.as<int32_t>(); pd.cell = g.cell.as<int32_t>(); pd.fx = g.fx.as<double>();
    pd.nslot = std::min(std::max(g.max_overlap, 1), (int)CS_CIA_ACT);
    pd.fac = g.fac.as<double>();
    pd.Tr = (cc.flags & CS_CIA_RADIATION) ? cc.st.Tr.as<double>() : nullptr;
    return pd;
}

// what the bands of slot cd fix on the column's grid: the band descriptors; for k_flux, room for ln k at every state's temperature, per
// tile the bands that reach it and per wavenumber its cell in each
static int cia_grid(cs_ctx *ctx, const CiaDev &cd, CiaGrid &g)
{
    const Column &c = ctx->col;
    const int nt64 = (int)((c.nnu + 63) / 64);
    g = CiaGrid();
    g.nband = (int)cd.bands.size();
    std::vector<CiaBand> hb(g.nband);
    std::vector<int64_t> toff(g.nband);
    int64_t tot = 0;
    for (int b = 0; b < g.nband; b++) {
        hb[b].nu = cd.bands[b].dnu.as<double>();
        hb[b].lnk = cd.bands[b].dlnk.as<double>();
        hb[b].nb = (int)cd.bands[b].nu.size();
        hb[b].nt = (int)cd.bands[b].T.size();
        toff[b] = tot;
        tot += (int64_t)c.K * hb[b].nb;
        g.maxnb = std::max(g.maxnb, hb[b].nb);
    }
    std::vector<int32_t> tband((size_t)nt64 * CS_CIA_ACT, -1);
    for (int ti = 0; ti < nt64; ti++) {
        const double vlo = c.h_nu[(int64_t)ti * 64], vhi = c.h_nu[std::min<int64_t>((int64_t)ti * 64 + 63, c.nnu - 1)];
        int n = 0;
        for (int b = 0; b < g.nband; b++)
            if (cd.bands[b].nu.front() <= vhi && cd.bands[b].nu.back() >= vlo) {
                if (n < CS_CIA_ACT) tband[(size_t)ti * CS_CIA_ACT + n] = b;
                n++;
            }
        g.max_overlap = std::max(g.max_overlap, n);
    }
    const int nslot = std::min(std::max(g.max_overlap, 1), (int)CS_CIA_ACT);
    std::vector<int32_t> cell((size_t)nslot * c.nnu, -1);
    std::vector<double> fx((size_t)nslot * c.nnu, 0.0);
    for (int ti = 0; ti < nt64; ti++)
        for (int q = 0; q < nslot; q++) {
            const int b = tband[(size_t)ti * CS_CIA_ACT + q];
            if (b < 0) continue;
            const std::vector<double> &v = cd.bands[b].nu;
            for (int64_t i = (int64_t)ti * 64; i < std::min<int64_t>((int64_t)ti * 64 + 64, c.nnu); i++) {
                const double x = c.h_nu[i];
                if (!(v.front() <= x && x <= v.back())) continue;      // Phi.G.xa <= nu <= Phi.G.xb, :255
                int lo = 0, hi = (int)v.size() - 1;                      // cell with v[lo] <= x < v[lo + 1] (the last one for x == v.back()): k_cia's search
                while (hi - lo > 1) { const int m = (lo + hi) >> 1; if (v[m] <= x) lo = m; else hi = m; }
                cell[(size_t)q * c.nnu + i] = lo;
                fx[(size_t)q * c.nnu + i] = (x - v[lo]) / (v[lo + 1] - v[lo]);
            }
        }
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = upload(g.bands, hb.data(), hb.size(), s)) || (rc = upload(g.toff, toff.data(), toff.size(), s)) ||
        (rc = upload(g.tband, tband.data(), tband.size(), s)) || (rc = upload(g.cell, cell.data(), cell.size(), s)) ||
        (rc = upload(g.fx, fx.data(), fx.size(), s)))
        return rc;
    HIPCHK(g.tab.reserve((size_t)tot * sizeof(double)));
    HIPCHK(g.fac.reserve((size_t)c.K * sizeof(double)));
    HIPCHK(hipStreamSynchronize(s));   // (the host vectors are locals)
    return CS_OK;
}

int cs_column_set_cia(cs_ctx *ctx, int ncia, const int *cia_slots, const int *flags, const double *P1, const double *P2)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    if (ncia < 0 || ncia > CS_MAX_CIA) return fail(CS_EINVAL, "ncia out of range");
    Column &c = ctx->col;
    HIPCHK(hipSetDevice(ctx->device));
    const int res = [&]() -> int {   // one way out: whatever fails in here, the column is left without pairs
        for (int t = 0; t < ncia; t++)
            if (cia_slots[t] < 0 || cia_slots[t] >= CS_MAX_CIA || !ctx->cia[cia_slots[t]].present)
                return fail(CS_EINVAL, "CIA slot %d is empty", cia_slots[t]);
        for (int t = 0; t < ncia && flags; t++)
            if (flags[t] & ~(CS_CIA_EXTRAPOLATE | CS_CIA_SINGLES | CS_CIA_RADIATION))
                return fail(CS_EINVAL, "CIA flags %d: only CS_CIA_EXTRAPOLATE, CS_CIA_SINGLES and CS_CIA_RADIATION are defined", flags[t]);
        // what depends on the grid and the tables alone (cia_grid) is kept while the pairs named are the ones the column already holds: an
        // RCM loop re-sets its pairs on every call for the partial pressures only
        bool same = (int)c.cia.size() == ncia;
        for (int t = 0; t < ncia && same; t++)
            same = c.cia[t].slot == cia_slots[t] && c.cia[t].generation == ctx->cia[cia_slots[t]].generation;
        if (!same) {
            drop_graph(c);
            c.cia.clear();
            c.cia.resize(ncia);
        }
        int rc;
        for (int t = 0; t < ncia; t++) {
            ColCia &cc = c.cia[t];
            const CiaDev &cd = ctx->cia[cia_slots[t]];
            const int fl = flags ? flags[t] : 0;
            if (same && ((fl ^ cc.flags) & CS_CIA_RADIATION)) drop_graph(c);   // (the captured launches name the kernels of the other kind)
            cc.slot = cia_slots[t];
            cc.flags = fl;
            cc.generation = cd.generation;
            if (!same && (rc = cia_grid(ctx, cd, cc.grid))) return rc;
            if ((rc = cia_states(ctx->stream, cd, fl, c.K, c.h_Tk.data(), c.h_Pk.data(), P1, P2, ncia, t, cc.st))) return rc;
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return CS_OK;
    }();
    if (res) c.cia.clear();
    return res;
}

static int sigma_impl(cs_ctx *ctx, hipStream_t s, hipEvent_t *ev, int &e, StepLog *log, bool *near_plane_live = nullptr, FluxFuse *fuse = nullptr, const FluxPlan *fpl = nullptr);
static int column_current(cs_ctx *ctx);

// ---- AcceleratedAbsorber (absorbers.jl:114-203) -------------------------------------------------------------------------
int cs_accel_store(cs_ctx *ctx, int accel_slot)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    if (accel_slot < 0 || accel_slot >= CS_MAX_ACCEL) return fail(CS_EINVAL, "accelerated-absorber slot %d out of range", accel_slot);
    Column &c = ctx->col;
    if (c.accel.slot >= 0) return fail(CS_ESTATE, "the resident column is itself an accelerated absorber");
    if (c.K < 2) return fail(CS_EINVAL, "need at least two pressure knots");
    for (int k = 1; k < c.K; k++)
        if (!(c.h_Pk[k] > c.h_Pk[k - 1])) return fail(CS_EORDER, "knot pressures must be strictly ascending");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int e = 0, rc;
    if ((rc = sigma_impl(ctx, s, nullptr, e, nullptr))) return rc;   // Sigma(U, i, T_k, P_k) for every i and knot k (update!, absorbers.jl:173-200)
    AccelDev &ad = ctx->accel[accel_slot];
    const int64_t n = (int64_t)c.K * c.nnu;
    HIPCHK(ad.L.reserve((size_t)n * sizeof(double)));
    CS_LAUNCH(k_accel_store, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, c.sigma.as<double>(), ad.L.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    std::vector<double> lnP(c.K);
    for (int k = 0; k < c.K; k++) lnP[k] = std::log(c.h_Pk[k]);
    if (!ad.present || ad.nnu != c.nnu || ad.nk != c.K || ad.lnP != lnP || ad.nu != c.h_nu) ad.generation = next_generation();   // other knots or grid (new values on the same ones: update!, absorbers.jl:173-200)
    ad.nnu = c.nnu;
    ad.nk = c.K;
    ad.nu = c.h_nu;
    ad.lnP = lnP;
    ad.present = true;
    return CS_OK;
}

int cs_accel_clear(cs_ctx *ctx, int accel_slot)
{
    if (!ctx || accel_slot < 0 || accel_slot >= CS_MAX_ACCEL) return fail(CS_EINVAL, "bad accelerated-absorber slot");
    if (ctx->col.accel.slot == accel_slot) { ctx->col.accel.slot = -1; ctx->col.ready = false; }
    ctx->accel[accel_slot] = AccelDev();
    return CS_OK;
}

// what the knots of ad need at N pressures: knot interval and abscissae of LinearInterpolator(lnP, y, NoBoundaries())(x), the cell of x
// clamped to the end cells (extrapolation)
static int accel_states(hipStream_t s, const AccelDev &ad, int N, const double *P, AccelStates &st)
{
    std::vector<int32_t> cell(N);
    std::vector<double> x(N), xa(N), xb(N);
    for (int k = 0; k < N; k++) {
        x[k] = std::log(P[k]);
        int i = (int)(std::upper_bound(ad.lnP.begin(), ad.lnP.end(), x[k]) - ad.lnP.begin()) - 1;
        i = std::min(std::max(i, 0), ad.nk - 2);
        cell[k] = i;
        xa[k] = ad.lnP[i];
        xb[k] = ad.lnP[i + 1];
    }
    int rc;
    if ((rc = upload(st.cell, cell.data(), N, s)) || (rc = upload(st.x, x.data(), N, s)) || (rc = upload(st.xa, xa.data(), N, s))) return rc;
    return upload(st.xb, xb.data(), N, s);   // (from pageable memory: the copies have left the host vectors on return)
}
// sigma[k][nu] = base (+ extra[k][nu]) + exp of the ln P-interpolated ln sigma, at N states (absorbers.jl:203)
static void launch_accel(hipStream_t s, const AccelDev &ad, const AccelStates &st, int N, double base, const double *extra, double *sigma)
{
    CS_LAUNCH(k_accel_eval, dim3((unsigned)((ad.nnu + 255) / 256), N), dim3(256), 0, s, ad.L.as<double>(), ad.nnu, N, st.cell.as<int32_t>(),
              st.x.as<double>(), st.xa.as<double>(), st.xb.as<double>(), base, extra, sigma);
}

int cs_accel_eval(cs_ctx *ctx, int accel_slot, double P, int64_t i0, int64_t n, double *sigma_out)
{
    if (!ctx || accel_slot < 0 || accel_slot >= CS_MAX_ACCEL || !ctx->accel[accel_slot].present) return fail(CS_EINVAL, "accelerated-absorber slot is empty");
    AccelDev &ad = ctx->accel[accel_slot];
    if (i0 < 0 || n < 1 || i0 + n > ad.nnu || !sigma_out) return fail(CS_EINVAL, "wavenumber range out of bounds");
    if (!(P > 0)) return fail(CS_EINVAL, "pressure must be positive");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = accel_states(s, ad, 1, &P, ctx->tmpAccel))) return rc;
    HIPCHK(ctx->tmpC.reserve((size_t)ad.nnu * sizeof(double)));
    launch_accel(s, ad, ctx->tmpAccel, 1, 0.0, nullptr, ctx->tmpC.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sigma_out, ctx->tmpC.as<double>() + i0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CS_OK;
}

int cs_column_set_accel(cs_ctx *ctx, int accel_slot)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    Column &c = ctx->col;
    drop_graph(c);
    if (accel_slot < 0) { c.accel.slot = -1; return CS_OK; }
    if (accel_slot >= CS_MAX_ACCEL || !ctx->accel[accel_slot].present) return fail(CS_EINVAL, "accelerated-absorber slot %d is empty", accel_slot);
    // an AcceleratedAbsorber stands for ALL absorbers of a column (unifyabsorbers(::Tuple{AcceleratedAbsorber}), absorbers.jl:216)
    if (c.ngas > 0 || !c.tab.empty() || !c.cia.empty()) return fail(CS_EINVAL, "a column over an accelerated absorber has no other absorbers");
    AccelDev &ad = ctx->accel[accel_slot];
    if (ad.nnu != c.nnu || !std::equal(ad.nu.begin(), ad.nu.end(), c.h_nu.begin())) return fail(CS_EINVAL, "wavenumber grids differ");
    HIPCHK(hipSetDevice(ctx->device));
    int rc;
    if ((rc = accel_states(ctx->stream, ad, c.K, c.h_Pk.data(), c.accel.st))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    c.accel.slot = accel_slot;
    c.accel.generation = ad.generation;
    return CS_OK;
}

int cs_column_setup(cs_ctx *ctx, int64_t nnu, const double *nu, const double *wts, int np, const double *P, double g,
                    int nlobatto, const double *T_nodes, const double *mu_nodes, const double *T_levels, int ngas,
                    const int *gas_slots, const int *shapes, const double *dnu_cuts, const double *conc,
                    double sigma_gray, const double *sigma_extra, const double *S_toa, const double *albedo,
                    double theta_s, int nstream, int want_tau, int want_M)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    Column &c = ctx->col;
    c.ready = false;
    c.F_dst = nullptr;      // (a destination for the band fluxes belongs to the column it was set for)
    drop_graph(c);
    if (np < 2) return fail(CS_EINVAL, "need at least two pressure levels");
    if (nlobatto < 2 || nlobatto > CS_MAX_LOBATTO) return fail(CS_EINVAL, "nlobatto must be in [2,%d]", CS_MAX_LOBATTO);
    if (nstream < 1 || nstream > CS_MAX_STREAM) return fail(CS_EINVAL, "nstream must be in [1,%d]", CS_MAX_STREAM);
    if (ngas < 0 || ngas > CS_MAX_GAS) return fail(CS_EINVAL, "ngas out of range");
    if (!(theta_s >= 0 && theta_s < M_PI / 2)) return fail(CS_EINVAL, "azimuth angle theta must be in [0,pi/2)");
    if (!(g > 0)) return fail(CS_EINVAL, "g must be positive");
    if ((int64_t)(np - 1) * (nlobatto - 1) + 1 > 65535) return fail(CS_EINVAL, "too many node states for one launch (65535)");
    int rc;
    if ((rc = check_ascending(nu, nnu))) return rc;
    for (int i = 1; i < np; i++)
        if (!(P[i] >= P[i - 1])) return fail(CS_EORDER, "pressure coordinates must be in ascending order (sorted)");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    c.nnu = nnu; c.np = np; c.nl = np - 1; c.nlob = nlobatto; c.K = (np - 1) * (nlobatto - 1) + 1;
    c.nstream = nstream; c.ngas = ngas; c.ntile = (int)((nnu + 255) / 256);
    c.flux = flux_plan(ctx->set, {nnu, np, nlobatto, c.K, nstream}, 1, nullptr);
    c.want_tau = want_tau == CS_TAU_NONE || want_tau == CS_TAU_TOTAL || want_tau == CS_TAU_TILES ? want_tau : CS_TAU_LAYERS;   // (any other non-zero value: layers)
    c.want_M = want_M == CS_M_NONE || want_M == CS_M_EDGES || want_M == CS_M_TILES ? want_M : CS_M_PLANES;   // (any other non-zero value: planes)
    c.g = g; c.sigma_gray = sigma_gray; c.theta_s = theta_s;
    const int K = c.K, nl = c.nl;
    // quadrature rules
    RtParams &rt = c.rt;
    memset(&rt, 0, sizeof rt);
    rt.np = np; rt.nlobatto = nlobatto; rt.K = K; rt.nstream = nstream;
    rt.mmode = c.want_M; rt.mtile = (int)c.m_ntile();   // (level_out: what the flux kernels store through the M pointers)
    rt.C = 1e-4 * kNa / g;
    rt.cos_ts = std::cos(theta_s);
    c.h_xs.assign(nlobatto, 0.0);
    cs_lobattonodes(nlobatto, c.h_xs.data(), rt.ws);
    cs_streamnodes(nstream, rt.m, rt.W);
    for (int k = 0; k < nstream; k++) rt.im[k] = 1.0 / rt.m[k];
    // node states: k = i*(nlobatto-1) + n   (discretized.jl:150,162,169)
    c.h_P.assign(P, P + np);
    c.h_nu.assign(nu, nu + nnu);
    c.h_Pk.assign(K, 0.0);
    c.h_Pk[0] = P[0];
    for (int i = 0; i < nl; i++) {
        const double dP = P[i + 1] - P[i];
        for (int n = 1; n < nlobatto; n++)
            c.h_Pk[i * (nlobatto - 1) + n] = (n == nlobatto - 1) ? P[i + 1] : P[i] + dP * c.h_xs[n];
    }
    std::vector<double> wt(nnu);
    if (wts) {
        std::copy(wts, wts + nnu, wt.begin());
    } else {  // trapz (util.jl:26-33) as per-point weights
        for (int64_t j = 0; j < nnu; j++) {
            double a = j > 0 ? nu[j] - nu[j - 1] : 0.0, b = j + 1 < nnu ? nu[j + 1] - nu[j] : 0.0;
            wt[j] = (a + b) / 2;
        }
    }
    if ((rc = upload(c.nu, nu, nnu, s)) || (rc = upload(c.wts, wt.data(), nnu, s)) || (rc = upload(c.P, P, np, s)) ||
        (rc = upload(c.Pk, c.h_Pk.data(), K, s)))
        return rc;
    c.default_wts = wts == nullptr;
    c.g_nnu = 0; c.g_start = 0; c.g_left = c.g_right = 0.0;   // (cs_fluxes_discretized_multi marks its shards after a successful setup)
    c.interp = interp_key(ctx);   // every setting of the context that shapes what setup builds
    c.has_extra = sigma_extra != nullptr;
    // an all-zero stellar spectrum / albedo is the same as none (0*exp(..) and M*0/pi are exact zeros): skip their work, and let
    // the upward sweep start without waiting for the downward one (k_rt<.., UD>)
    c.has_S = S_toa != nullptr && std::any_of(S_toa, S_toa + nnu, [](double x) { return x != 0.0; });
    c.has_alb = albedo != nullptr && std::any_of(albedo, albedo + nnu, [](double x) { return x != 0.0; });
    if (c.has_extra && (rc = upload(c.extra, sigma_extra, (size_t)nnu * K, s))) return rc;
    if (c.has_S && (rc = upload(c.S_toa, S_toa, nnu, s))) return rc;
    if (c.has_alb && (rc = upload(c.albedo, albedo, nnu, s))) return rc;
    // gases: launch groups, tile windows and workspace
    c.gas.clear();
    c.ugas.clear();
    c.ugas.resize(ngas);
    c.merge = ctx->merge;
    c.grid_id = ++g_grid_counter;
    c.cheb.nlev = 0;
    c.cheb.nItot = 0;    // (cs_column_work reports it: no intervals of the column this one replaces)
    if (ctx->interp) {   // interval sizes from the narrowest Voigt cut-off of the column
        double cmin = 0.0;
        for (int gi = 0; gi < ngas; gi++) {
            if (shape_spec(shapes ? shapes[gi] : CS_SHAPE_VOIGT).voigt_family()) {   // (a flagged Voigt / Lorentz gas interpolates its far wings too)
                const double cu = dnu_cuts ? dnu_cuts[gi] : 25.0;
                cmin = cmin > 0.0 ? std::min(cmin, cu) : cu;
            }
        }
        if (cmin > 0.0 && (rc = cheb_build(ctx, c.cheb, nu, c.nu.as<double>(), nnu, cmin, s))) return rc;
    }
    std::vector<std::vector<int>> groups;
    for (int gi = 0; gi < ngas; gi++) {
        UserGas &ug = c.ugas[gi];
        ug.slot = gas_slots[gi];
        ug.shape = shapes ? shapes[gi] : CS_SHAPE_VOIGT;
        ug.cut = dnu_cuts ? dnu_cuts[gi] : 25.0;
        if (ug.slot < 0 || ug.slot >= CS_MAX_GAS || !ctx->gas[ug.slot].present)
            return fail(CS_EINVAL, "gas slot %d is empty", ug.slot);
        ug.generation = ctx->gas[ug.slot].generation;
        ShapeSpec sh;
        if ((rc = decode_shape(ug.shape, sh))) return rc;
        const GasTable &G = ctx->gas[ug.slot];
        double ds_unused;
        if (sh.pshift && (rc = shift_width(G, P, np, ds_unused))) return rc;
        ug.pairs_per_state = -1;   // counted on demand (cs_column_counts): O(nnu log L) on the host
        ug.lines_in_range = std::upper_bound(G.h_nu.begin(), G.h_nu.end(), nu[nnu - 1] + ug.cut) -
                            std::lower_bound(G.h_nu.begin(), G.h_nu.end(), nu[0] - ug.cut);   // (the reference's count: inside the cut-off)
        // Voigt (Lorentz, pedestal-removed Voigt, Van Vleck-Huber Voigt, both) gases with the same shape and cut-off go into one group --
        // never codes 4, 5, 6 with code 0 or with each other: the pedestal, or R(nu, T) and the mirror term, act on every line of a group; a
        // slot named twice stays apart (a merged table tags a line with ONE member).  ug.shape is the caller's code, CS_SHAPE_PSHIFT included:
        // a flagged group merges only with flagged gases of the same base code and cut-off
        bool placed = false;
        if (ctx->merge && sh.voigt_family())
            for (auto &grp : groups) {
                const UserGas &h = c.ugas[grp[0]];
                bool dup = false;
                for (int m : grp) dup = dup || c.ugas[m].slot == ug.slot;
                if (h.shape == ug.shape && h.cut == ug.cut && !dup && grp.size() < 255) { grp.push_back(gi); placed = true; break; }
            }
        if (!placed) groups.push_back(std::vector<int>{gi});
    }
    // code-5 and code-6 groups first: each runs on its own (no deferred node-sum apply, no side streams: R(nu, T) multiplies everything its
    // line sum adds) and the first one's sum is the plane itself; the groups after them share the deferred apply and the near-line plane as before
    std::stable_partition(groups.begin(), groups.end(), [&](const std::vector<int> &g) { return shape_spec(c.ugas[g[0]].shape).vvh; });
    c.gas.resize(groups.size());
    c.maxL = 0;
    c.any_ped = c.has_phco2 = false;
    bool any_voigt = false;
    for (size_t qi = 0; qi < groups.size(); qi++) {
        ColGas &cg = c.gas[qi];
        cg.mem = groups[qi];
        const ShapeSpec sh = shape_spec(c.ugas[cg.mem[0]].shape);
        cg.shape = sh.line_shape;   // codes 4, 5, 6: every kernel of a Voigt group, then the pedestal and / or R(nu, T) and the mirror term
        cg.pshift = sh.pshift; cg.ped = sh.ped; cg.vvh = sh.vvh;
        cg.cut = c.ugas[cg.mem[0]].cut;
        if (cg.mem.size() == 1) {
            cg.tab = &ctx->gas[c.ugas[cg.mem[0]].slot];
        } else {
            std::vector<int> slots;
            for (int m : cg.mem) slots.push_back(c.ugas[m].slot);
            if ((rc = merged_table(ctx, slots, &cg.hold))) return rc;
            cg.tab = cg.hold.get();
        }
        const GasTable &G = *cg.tab;
        double ds = 0.0;   // CS_SHAPE_PSHIFT: windows and line range widened by the group's largest shift at the node pressures
        if (sh.pshift && (rc = shift_width(G, c.h_Pk.data(), K, ds))) return rc;
        if (cg.shape == SH_VOIGT && (rc = check_near_density(G, nu, nnu, cg.cut, ds))) return rc;
        if ((rc = build_windows(cg.w, G, sh, cg.cut, ds, nu, nnu, false, s))) return rc;
        HIPCHK(cg.zones.reserve((size_t)c.K * cg.w.nwin * sizeof(Zone)));
        HIPCHK(cg.st.gmax.reserve((size_t)c.K * sizeof(double)));
        if (c.cheb.nlev > 0 && sh.voigt_family() &&
            (rc = gas_interp_build(ctx, cg.itp, c.cheb, G.h_nu, cg.w.g0, cg.w.g1, nu, nnu, cg.cut, c.K, s, false, cg.w.ds)))
            return rc;
        c.maxL = std::max(c.maxL, (size_t)G.L);
        any_voigt = any_voigt || cg.shape == SH_VOIGT;
        c.any_ped = c.any_ped || cg.ped;
        c.has_phco2 = c.has_phco2 || cg.shape == SH_PHCO2;
    }
    if (c.cheb.nlev > 0) {
        const size_t fb = (size_t)c.cheb.nItot * CS_NC * cheb_kpad(K) * sizeof(double);
        if (c.chebF.bytes < fb) {
            HIPCHK(c.chebF.reserve(fb));
            HIPCHK(hipMemsetAsync(c.chebF.p, 0, c.chebF.bytes, s));   // padding states stay finite
        }
    }
    // (the fp32 records of mixed precision are sized when a step first needs them: sigma_impl; the spare plane: a second code-5 group)
    if ((rc = reserve_lines(K, c.maxL, nnu, c.hot, c.cold, ngas > 0 ? &c.ranges : nullptr, nullptr, c.any_ped ? &c.ped : nullptr,
                            c.gas.size() > 1 && c.gas[1].vvh ? &c.vvh : nullptr)))
        return rc;
    HIPCHK(c.sigma.reserve((size_t)K * nnu * sizeof(double)));
    if (any_voigt) HIPCHK(c.sigma2.reserve((size_t)K * nnu * sizeof(double)));
    // the caller's output, or k_flux_chunk's scratch between its two sweeps; a column in a depth mode runs form 0 and stores no layer depths:
    // k_depth's product instead, [nnu] or [np][ntile]
    if (!c.depth_mode()) HIPCHK(c.tau.reserve((size_t)nl * nnu * sizeof(double)));
    else HIPCHK(c.depth.reserve((c.want_tau == CS_TAU_TOTAL ? (size_t)nnu : (size_t)np * (size_t)c.m_ntile()) * sizeof(double)));
    if (!c.ticket.p) {
        HIPCHK(c.ticket.reserve((size_t)(1 + 512 / CS_FLUX_GROUP) * sizeof(unsigned)));
        HIPCHK(hipMemsetAsync(c.ticket.p, 0, c.ticket.bytes, s));
    }
    if (c.want_M) {   // by mode: [np][nnu], [2][nnu] or [np][ntile] -- the planes only for a column that asked for them
        const size_t mbytes = (size_t)c.m_rows() * (size_t)c.m_cols() * sizeof(double);
        HIPCHK(c.Mup.reserve(mbytes));
        HIPCHK(c.Mdn.reserve(mbytes));
    }
    HIPCHK(c.partial.reserve(c.flux.npartial * 2 * np * sizeof(double)));
    HIPCHK(c.F.reserve((size_t)2 * np * sizeof(double)));
    HIPCHK(hipStreamSynchronize(s));
    c.ready = true;  // state upload below needs the sizes
    c.tab.clear();
    c.cia.clear();
    c.accel.slot = -1;
    if ((rc = cs_column_update_state(ctx, T_nodes, mu_nodes, T_levels, conc, nullptr))) { c.ready = false; return rc; }
    return CS_OK;
}

// node states (discretized.jl:150,162,169) of B sets of T_nodes / mu_nodes [nl][nlob], one after the other: Tk, muk [B][K]
static void unpack_nodes(const Column &c, int B, const double *T_nodes, const double *mu_nodes, std::vector<double> &Tk, std::vector<double> &muk)
{
    const int K = c.K, q = c.nlob - 1;   // state 0 is node 0 of layer 0, state k > 0 node (k - 1) % q + 1 of layer (k - 1) / q
    Tk.resize((size_t)B * K);
    muk.resize((size_t)B * K);
    for (int b = 0; b < B; b++)
        for (int k = 0; k < K; k++) {
            const size_t j = (size_t)b * c.nlob * c.nl + (k ? (size_t)((k - 1) / q) * c.nlob + (k - 1) % q + 1 : 0);
            Tk[(size_t)b * K + k] = T_nodes[j];
            muk[(size_t)b * K + k] = mu_nodes[j];
        }
}

int cs_column_update_state(cs_ctx *ctx, const double *T_nodes, const double *mu_nodes, const double *T_levels,
                           const double *conc, const double *conc_tab)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    Column &c = ctx->col;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int K = c.K;
    std::vector<double> Tk, muk;
    unpack_nodes(c, 1, T_nodes, mu_nodes, Tk, muk);
    int rc;
    c.h_Tk = Tk;
    for (int gi = 0; gi < c.ngas; gi++)
        if ((rc = check_gas_states(ctx->gas[c.ugas[gi].slot], K, Tk.data()))) return rc;
    if ((rc = upload(c.Tk, Tk.data(), K, s)) || (rc = upload(c.muk, muk.data(), K, s)) ||
        (rc = upload(c.Tlev, T_levels, c.np, s)))
        return rc;
    for (auto &cg : c.gas) {
        if ((rc = column_group_states(ctx, cg, cg.st, K, Tk.data(), c.h_Pk.data(), conc, s))) return rc;
        if (cg.shape != SH_PHCO2) continue;
        // a PHCO2 group's levels carry the regions its states allow: a captured step holds the launches of one such choice
        const int mask = ph_wide_regions(cg.st.h_T.data(), cg.st.h_gmax.data(), K, cg.cut);
        if (mask != cg.ph_mask) drop_graph(c);
        cg.ph_mask = mask;
    }
    HIPCHK(hipStreamSynchronize(s));
    if (!c.tab.empty()) {
        if (!conc_tab) return fail(CS_EINVAL, "the resident column has opacity tables: conc_tab is required");
        if ((rc = upload_tables(ctx, conc_tab))) return rc;
    }
    return CS_OK;
}

// what a launch group of the resident column fixes at setup: its table, record range and shape, the grid and its windows, and how the
// context runs it; the callers add the states, the workspace and the output (one state set of the column | a chunk of a batch).
// hot32: the caller's fp32 records (the column's own | the batch's), used under mixed precision
static GasPass column_pass(cs_ctx *ctx, const ColGas &cg, const DevBuf &hot32)
{
    const Column &c = ctx->col;
    GasPass p;
    p.G = cg.tab; p.shape = cg.shape; p.cut = cg.cut; p.ped = cg.ped; p.vvh = cg.vvh; p.pshift = cg.pshift;
    pass_windows(p, cg.w);
    p.dnu = c.nu.as<double>(); p.nu = c.h_nu.data(); p.nnu = c.nnu;
    p.hot32 = (ctx->mixed && cg.shape == SH_VOIGT) ? hot32.as<LineF32>() : nullptr;
    p.base = c.sigma_gray;   // (clamp stays off: the column's sigma is complete only after its last absorber)
    p.far_s = ctx->far_s; p.ph = &ctx->ph;
    return p;
}

int cs_column_batch(cs_ctx *ctx, int B, const double *T_nodes, const double *mu_nodes, const double *T_levels,
                    const double *conc, const double *conc_tab, const double *cia_P1, const double *cia_P2, double *Fup, double *Fdn)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    Column &c = ctx->col;
    if (B < 1 || B > 65535) return fail(CS_EINVAL, "batch size must be in [1, 65535]");
    {
        const int rc0 = column_current(ctx);
        if (rc0) return rc0;
    }
    if (!c.tab.empty() && !conc_tab) return fail(CS_EINVAL, "the resident column has opacity tables: conc_tab is required");
    if (!c.cia.empty() && (!cia_P1 || !cia_P2)) return fail(CS_EINVAL, "the resident column has CIA pairs: cia_P1 and cia_P2 are required");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const int K = c.K, np = c.np;
    const int64_t BK = (int64_t)B * K;
    std::vector<double> Tk, muk, Pk(BK);
    unpack_nodes(c, B, T_nodes, mu_nodes, Tk, muk);
    for (int b = 0; b < B; b++) std::copy(c.h_Pk.begin(), c.h_Pk.end(), Pk.begin() + (size_t)b * K);
    int rc;
    for (int gi = 0; gi < c.ngas; gi++)
        if ((rc = check_gas_states(ctx->gas[c.ugas[gi].slot], (int)BK, Tk.data()))) return rc;
    const double *extra = c.has_extra ? c.extra.as<double>() : nullptr;
    if (extra) return fail(CS_EINVAL, "host-evaluated sigma(nu,T,P) terms are not supported in batch mode");
    const bool shared_sigma = c.accel.slot >= 0;   // AcceleratedAbsorber: cross-sections do not depend on the thermal state (absorbers.jl:203)
    DevBuf dped, dvvh, dTk, dPk, dmuk, dTlev, dsig, dtau, dpart, dF, dranges, dzones, dizones, dF2, dsep, dedge, hot, cold, hot32;
    GroupStates st;   // of one group at all B K states: the next group's take their place
    TabStates tst; CiaStates cst;   // ... and of one table, of one CIA pair
    if ((rc = upload(dTk, Tk.data(), BK, s)) || (rc = upload(dPk, Pk.data(), BK, s)) || (rc = upload(dmuk, muk.data(), BK, s)) ||
        (rc = upload(dTlev, T_levels, (size_t)B * np, s)))
        return rc;
    const FluxPlan bg = flux_plan(ctx->set, {c.nnu, np, c.nlob, K, c.nstream}, B, nullptr);
    if (!shared_sigma) HIPCHK(dsig.reserve((size_t)BK * c.nnu * sizeof(double)));
    HIPCHK(dpart.reserve(bg.npartial * 2 * np * sizeof(double)));
    HIPCHK(dF.reserve((size_t)B * 2 * np * sizeof(double)));
    double *sig = shared_sigma ? c.sigma.as<double>() : dsig.as<double>();
    StepLog log;
    if (shared_sigma) {
        int e = 0;
        if ((rc = sigma_impl(ctx, s, nullptr, e, &log))) return rc;
    } else if (c.ngas == 0) {
        const int64_t tot = BK * c.nnu;
        CS_LAUNCH(k_fill, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, tot, c.sigma_gray, (const double *)nullptr, sig);
    }
    const size_t maxL = c.maxL;
    const bool any_ped = c.any_ped;
    const bool vvh2 = c.gas.size() > 1 && c.gas[1].vvh;   // a second code-5 group: its line sum goes to a plane of its own first
    const size_t per_state = maxL * (sizeof(LineHot) + sizeof(LineCold) + (ctx->mixed ? sizeof(LineF32) : 0)) + (size_t)c.nnu * kNearPointBytes +
                             (any_ped ? ped_bytes(1, (int64_t)maxL) : 0) + (vvh2 ? (size_t)c.nnu * sizeof(double) : 0);
    const int kc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)BK, ((size_t)8 << 30) / std::max<size_t>(per_state, 1), (size_t)65535}));
    if (c.ngas > 0 && (rc = reserve_lines(kc, maxL, c.nnu, hot, cold, &dranges, ctx->mixed ? &hot32 : nullptr, any_ped ? &dped : nullptr,
                                          vvh2 ? &dvvh : nullptr)))
        return rc;
    if (c.has_phco2) ph_set_grid(ctx, c.h_nu.data(), c.nnu, c.grid_id);
    for (size_t qi = 0; qi < c.gas.size(); qi++) {
        ColGas &cg = c.gas[qi];
        const size_t nt64 = (size_t)((c.nnu + 63) / 64);
        if ((rc = column_group_states(ctx, cg, st, BK, Tk.data(), Pk.data(), conc, s))) return rc;
        HIPCHK(dzones.reserve((size_t)kc * nt64 * sizeof(Zone)));
        GasPass p = column_pass(ctx, cg, hot32);
        p.mstride = (int)BK;
        p.hot = hot.as<LineHot>(); p.cold = cold.as<LineCold>(); p.zones = dzones.as<Zone>(); p.ranges = dranges.as<unsigned>(); p.ped_ws = dped.as<double>();
        p.accumulate = qi > 0; p.spare = dvvh.as<double>();   // (a second code-5/6 group: its bare line sum goes there first)
        p.log = &log;
        Interp &itp = p.itp;
        if (cg.itp.nlev > 0) {
            HIPCHK(dizones.reserve((size_t)kc * c.cheb.nItot * sizeof(IZone)));
            const size_t fb = (size_t)c.cheb.nItot * CS_NC * cheb_kpad(kc) * sizeof(double);
            if (dF2.bytes < fb) {
                HIPCHK(dF2.reserve(fb));
                HIPCHK(hipMemsetAsync(dF2.p, 0, dF2.bytes, s));
            }
            itp = interp_view(c.cheb, cg.itp, kc, dizones.as<IZone>());
            itp.F = dF2.as<double>();
            HIPCHK(dsep.reserve((size_t)((kc + 15) / 16) * c.cheb.nItot * sizeof(SepZone)));   // (the column's own buffer is sized for K states)
            HIPCHK(dedge.reserve((size_t)((kc + 15) / 16) * nt64 * sizeof(EdgeZone)));
            itp.sep = dsep.as<SepZone>();
            itp.edge = dedge.as<EdgeZone>();
            interp_select(ctx, itp);
            p.set = &ctx->set;
        }
        for (int64_t k0 = 0; k0 < BK; k0 += kc) {
            p.kn = (int)std::min<int64_t>(kc, BK - k0);
            p.Tk = dTk.as<double>() + k0; p.Pk = dPk.as<double>() + k0; p.scale = st.conc.as<double>() + k0;
            pass_states(p, st, k0);
            p.sigma = sig + (size_t)k0 * c.nnu;
            launch_gas(s, p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(s));   // the device buffers are reused by the next group
    }
    // baked gases of the column at all B*K states: the Gas functor fC(T,P)*exp(Phi(T, ln P)) (gases.jl:85,278) -- what RCM holds
    // inside its AcceleratedAbsorber (radiative_convective.jl:6-103)
    const int nt = shared_sigma ? 0 : (int)c.tab.size(), nc = shared_sigma ? 0 : (int)c.cia.size();
    for (int t = 0; t < nt; t++) {
        const TableDev &tb = ctx->tab[c.tab[t].slot];
        if ((rc = table_states(s, tb, BK, Tk.data(), Pk.data(), conc_tab, nt, t, tst))) return rc;
        if ((rc = launch_table_eval(s, tb, tst, (int)BK, sig))) return rc;
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));   // the record is reused by the next table
    }
    // its CIA pairs: the partial pressures of pair t at state b K + k are element t + nc (b K + k) of the caller's [B][nc * K] rows
    for (int t = 0; t < nc; t++) {
        if ((rc = cia_states(s, ctx->cia[c.cia[t].slot], c.cia[t].flags, (int)BK, Tk.data(), Pk.data(), cia_P1, cia_P2, nc, t, cst))) return rc;
        launch_cia(s, c, c.cia[t], cst, (int)BK, sig);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(s));
    }
    log.disp.flags |= bg.flags;
    c.log_last.disp = log.disp;
    const FluxArgs fa = {&c.rt, c.nu.as<double>(), c.wts.as<double>(), c.nnu, sig, dmuk.as<double>(), c.P.as<double>(), dTlev.as<double>(),
                         c.has_S ? c.S_toa.as<double>() : nullptr, c.has_alb ? c.albedo.as<double>() : nullptr,
                         nullptr, nullptr, nullptr, dpart.as<double>(), s};   // batches return band fluxes only: no tau stored
    if ((rc = launch_flux(bg, B, fa, shared_sigma ? 0 : (size_t)K * c.nnu, nullptr))) return rc;
    CS_LAUNCH(k_freduce, dim3(2 * np, B), dim3(256), 0, s, dpart.as<double>(), bg.nfreduce, 2 * np, dF.as<double>());
    HIPCHK(hipGetLastError());
    std::vector<double> F((size_t)B * 2 * np);
    HIPCHK(hipMemcpyAsync(F.data(), dF.p, F.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int b = 0; b < B; b++) {
        std::copy(F.begin() + (size_t)b * 2 * np, F.begin() + (size_t)b * 2 * np + np, Fup + (size_t)b * np);
        std::copy(F.begin() + (size_t)b * 2 * np + np, F.begin() + (size_t)(b + 1) * 2 * np, Fdn + (size_t)b * np);
    }
    return CS_OK;
}

// the cross-section stage of one evaluation: sigma[K][nnu] of all absorbers of the resident column at its node states
// (Sigma(A, i, T, P) of absorbers.jl:95 for every i and node).  ev: see run_impl; e counts the events recorded.  log: the step's record, or NULL.
// near_plane_live: NULL = the cross-sections themselves are the result (the near-line plane is folded into sigma before returning);
// else the caller (run_impl) hands both planes to k_rt and is told here whether the second one is in use this step
// fuse != NULL: the interpolated wings are not carried to the grid and the CIA pairs are not added here -- *fuse says what the flux
// kernel still has to add (k_flux; near_plane_live must be given too: the near-line plane is not folded in either), and *fpl is the step's flux plan
static int sigma_impl(cs_ctx *ctx, hipStream_t s, hipEvent_t *ev, int &e, StepLog *log, bool *near_plane_live, FluxFuse *fuse, const FluxPlan *fpl)
{
    Column &c = ctx->col;
    const int K = c.K;
    {
        const int rc0 = column_current(ctx);
        if (rc0) return rc0;
    }
    double *sig = c.sigma.as<double>();
    const double *extra = c.has_extra ? c.extra.as<double>() : nullptr;
    if (c.accel.slot >= 0) {   // AcceleratedAbsorber: exp of the ln P-interpolated ln sigma (absorbers.jl:203)
        launch_accel(s, ctx->accel[c.accel.slot], c.accel.st, K, c.sigma_gray, extra, sig);   // (its grid is the column's: cs_column_set_accel)
    } else if (c.gas.empty()) {
        const int64_t tot = (int64_t)K * c.nnu;
        CS_LAUNCH(k_fill, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, tot, c.sigma_gray, extra, sig);
    }
    if (ctx->mixed) HIPCHK(c.hot32.reserve(((size_t)K * c.maxL + 4) * sizeof(LineF32)));   // no-op once sized (not capturable the first time)
    ChebApply apply;
    apply.ngas = 0;
    if (c.has_phco2) ph_set_grid(ctx, c.h_nu.data(), c.nnu, c.grid_id);
    int n_itp = 0;
    for (auto &cg : c.gas) n_itp += cg.itp.nlev > 0 && !cg.vvh ? 1 : 0;   // (the groups whose node sums go into the deferred apply)
    // Settings::nodes_stream: node sums on a side stream -- 1: where the grid is short (fewer than 16384 (tile, state) waves), 2: always
    // Settings::near_stream: the near-line kernels on a second side stream, into a plane of their own (1, default; 0: after k_voigt_edge_mx, into sigma)
    Fork fk;
    memset(&fk, 0, sizeof fk);
    fk.s2 = ctx->stream2; fk.ev_fork = ctx->ev_fork; fk.ev_join = ctx->ev_join;
    fk.s3 = ctx->stream3; fk.ev_fork3 = ctx->ev_fork3; fk.ev_join3 = ctx->ev_join3; fk.ev_far3 = ctx->ev_far3;
    fk.use_nodes = !ev && (ctx->set.nodes_stream == 2 || (ctx->set.nodes_stream == 1 && (c.nnu + 63) / 64 * (int64_t)K < 16384));
    // (1 = where it was measured to pay: 1/8 shards of C3 -3..-6 %, C3 -1 %; not on tiny columns -- C2 +19 %: the join costs more than
    //  the kernels -- nor on very long sparse ones -- C5 +2 %; 2 = always)
    const int64_t tswaves = (c.nnu + 63) / 64 * (int64_t)K;
    fk.use_near = !ev && c.sigma2.p != nullptr && (ctx->set.near_stream == 2 || (ctx->set.near_stream == 1 && tswaves >= 8192 && tswaves <= 300000));
    fk.sigma2 = fk.use_near ? c.sigma2.as<double>() : nullptr;
    const bool use_fork = fk.use_nodes || fk.use_near;
    for (int gi = 0; gi < (int)c.gas.size(); gi++) {
        ColGas &cg = c.gas[gi];
        GasPass p = column_pass(ctx, cg, c.hot32);
        p.kn = K;
        p.Tk = c.Tk.as<double>(); p.Pk = c.Pk.as<double>(); p.scale = cg.st.conc.as<double>(); p.mstride = K;
        pass_states(p, cg.st, 0);
        p.hot = c.hot.as<LineHot>(); p.cold = c.cold.as<LineCold>(); p.zones = cg.zones.as<Zone>(); p.ranges = c.ranges.as<unsigned>(); p.ped_ws = c.ped.as<double>();
        // (code 4: the pedestal comes off the plane the group's first kernel initialised; the near-line plane and the wings still to come only add)
        p.extra = extra; p.sigma = sig; p.accumulate = gi > 0; p.spare = c.vvh.as<double>();
        if (cg.itp.nlev > 0) p.itp = interp_view(c.cheb, cg.itp, K);
        p.itp.F = c.chebF.as<double>();
        interp_select(ctx, p.itp);
        p.set = &ctx->set;
        p.fuse_apply = ctx->set.fuse_apply && n_itp == 1;
        p.defer = &apply; p.fork = use_fork ? &fk : nullptr; p.evg = ev ? ev + e : nullptr;
        p.log = log;
        const bool voigt = cg.shape == SH_VOIGT || cg.shape == SH_LORENTZ;   // (what line_sum_voigt runs, and plans)
        p.keep = voigt ? &cg.plan : nullptr;
        launch_gas(s, p);
        cg.planned = voigt;
        if (ev) { e += 6; HIPCHK(hipEventRecord(ev[e++], s)); }
    }
    if (fuse) { fuse->apply = 0; fuse->ncia = 0; fuse->Kpad = cheb_kpad(K); }
    // short grids with the node sums on their side stream: that stream has slack (it ends well before the per-point kernels), so the levels
    // are folded into the smallest one THERE (k_cheb_cascade, exact to rounding) and the flux kernel carries one level to the grid instead
    // of three -- one memory latency in its first phase instead of three (13 -> 6 us on a 1/8 shard of the bench column)
    bool cascaded_aside = false;
    ChebApply carried;   // what a cascade on the side stream leaves to carry to the grid
    const int nl_itp = apply.ngas == 1 ? apply.nlev - apply.l0[0] : 0;
    const bool short_aside = fuse && fpl->rt_kern == FK_RT_STREAMS;
    // long grids: where the cascade is in use anyway (four levels and up) it runs on the node-sum stream as well, beside the per-point
    // kernels, instead of between them and the flux kernel (BASELINE configs[4]: four launches, 0.32 ms of the main stream)
    // ... and with the node sums on a side stream the cascade is off the step's critical path whatever the number of levels: that stream
    // ends long before the other two at full size (the bench column: 1.34 against 1.60 and 1.86 ms into the step), so folding three levels
    // into one there makes the carry to the grid a third of its matrix products and of its reads of C (round 5: 1.880 -> 1.872 ms)
    const bool casc_on = nl_itp >= 2 && ctx->set.cascade != 2 && (ctx->set.cascade == 1 || cascade_pays(nl_itp) || fk.pending);
    if (apply.ngas == 1 && fk.pending && !ctx->set.no_cascade_aside && nl_itp >= 2 && (short_aside || casc_on)) {
        const double *Rc[CS_MAX_LEVEL];
        for (int l = 0; l < CS_MAX_LEVEL; l++) Rc[l] = c.cheb.Rc[l].as<double>();
        launch_apply_cascade(fk.s2, apply, Rc, c.cheb.itv, c.cheb.nI, 1, cheb_kpad(K), c.nnu, K, 0.0, nullptr, sig, 1, &carried);
        (void)hipEventRecord(fk.ev_join, fk.s2);   // (the main stream has not waited yet: it will wait for this later record)
        cascaded_aside = true;
        if (log) log->disp.flags |= CS_DF_CASCADE_ASIDE;
    }
    fork_join(&fk, s, true, false);   // the node sums; the near-line kernels may run on beside what follows (none of it touches their plane)
    // interpolated far wings of all gases: sigma += sum_level C (sum_gas F)  (one pass over C and sigma)
    if (apply.ngas > 0 && cascaded_aside) {
        if (fuse) { fuse->A = carried; fuse->apply = 1; }
        else launch_apply(s, carried, cheb_kpad(K), c.nnu, K, 0.0, nullptr, sig, 1);
    } else if (apply.ngas > 0) {
        const double *Rc[CS_MAX_LEVEL];
        for (int l = 0; l < CS_MAX_LEVEL; l++) Rc[l] = c.cheb.Rc[l].as<double>();
        launch_apply_cascade(s, apply, Rc, c.cheb.itv, c.cheb.nI, ctx->set.cascade, cheb_kpad(K), c.nnu, K, 0.0, nullptr, sig, 1,
                             fuse ? &fuse->A : nullptr);
        if (fuse) fuse->apply = 1;
    }
    for (auto &t : c.tab)  // baked gases: sigma += fC * exp(Phi(T, ln P))
        if (const int rc2 = launch_table_eval(s, ctx->tab[t.slot], t.st, K, sig)) return rc2;
    for (auto &cc : c.cia) {  // CIA pairs
        if (fuse) {   // the temperature half of the interpolation per (band, state, sample); k_flux does the rest per point
            const CiaPairDev &pd = fuse->cia[fuse->ncia++] = cia_pair(cc);
            CS_LAUNCH(k_cia_tab, dim3((unsigned)((cc.grid.maxnb + 255) / 256), (unsigned)K, (unsigned)cc.grid.nband), dim3(256), 0, s, pd, K);
            continue;
        }
        launch_cia(s, c, cc, cc.st, K, sig);
    }
    fork_join(&fk, s);
    c.near_live = false;
    c.sigma_partial = fuse != nullptr;
    if (near_plane_live) *near_plane_live = fk.live;
    else if (fk.live) {
        const int64_t tot = (int64_t)K * c.nnu;
        CS_LAUNCH(k_fold, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, tot, sig, c.sigma2.as<double>());
    }
    if (!near_plane_live) {   // the cross-sections are the result: complete here, so the max(0, .) of a code-4 or code-6 group applies
        const int64_t tot = (int64_t)K * c.nnu;
        if (c.any_ped) CS_LAUNCH(k_clamp0, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, tot, sig);
    }
    HIPCHK(hipGetLastError());
    return CS_OK;
}

// a table re-uploaded into (or cleared from) a slot of the resident column leaves its windows stale: refuse to run on them
static int column_current(cs_ctx *ctx)
{
    Column &c = ctx->col;
    // the slot still holds what the column formed its windows, weights, cells or per-grid tables from
    auto slot_current = [](const auto &sl, uint64_t generation) { return sl.present && sl.generation == generation; };
    for (auto &ug : c.ugas)
        if (!slot_current(ctx->gas[ug.slot], ug.generation)) {
            c.ready = false;
            return fail(CS_ESTATE, "gas slot %d was re-uploaded or cleared after cs_column_setup", ug.slot);
        }
    // the same for the opacity tables and the accelerated absorber the column names by slot: its weights [nT * nP][K] / knot cells were
    // formed for the (T, P) grid / knots the slot held at cs_column_set_tables / cs_column_set_accel
    for (auto &ct : c.tab)
        if (!slot_current(ctx->tab[ct.slot], ct.generation))
            return fail(CS_ESTATE, "opacity-table slot %d was baked, uploaded or cleared after cs_column_set_tables: call it again", ct.slot);
    if (c.accel.slot >= 0 && !slot_current(ctx->accel[c.accel.slot], c.accel.generation))
        return fail(CS_ESTATE, "accelerated-absorber slot %d got other knots (or was cleared) after cs_column_set_accel: call it again", c.accel.slot);
    // ... and for the CIA pairs: their band descriptors hold the addresses of the slot's tables as cs_column_set_cia found them, and
    // cs_cia_begin / cs_cia_clear free those
    for (auto &cc : c.cia)
        if (!slot_current(ctx->cia[cc.slot], cc.generation))
            return fail(CS_ESTATE, "CIA slot %d got other bands (or was cleared) after cs_column_set_cia: call it again", cc.slot);
    return CS_OK;
}

// the column's slant optical depth, or its per-tile transmittances to space (CS_TAU_TOTAL / CS_TAU_TILES), from the cross-section plane as the
// call in progress leaves it: one wave per 64-point tile
static void launch_depth(Column &c, hipStream_t s, const double *sigma2)
{
    const int64_t nt64 = c.m_ntile();
    CS_LAUNCH(k_depth, dim3((unsigned)((nt64 + 3) / 4)), dim3(256), 0, s, c.rt, c.nu.as<double>(), c.wts.as<double>(), c.nnu, c.sigma.as<double>(), sigma2,
              c.muk.as<double>(), c.P.as<double>(), c.want_tau, c.depth.as<double>());
}

// enqueue one evaluation; when ev != NULL an event is recorded between the kernel classes (ev must hold 7 * (launch groups) + 4)
static int run_impl(cs_ctx *ctx, hipStream_t s, hipEvent_t *ev)
{
    Column &c = ctx->col;
    double *sig = c.sigma.as<double>();
    int e = 0, rc;
    g_nlaunch = 0;
    StepLog log;
    c.last_stream = s;
    if (ev) HIPCHK(hipEventRecord(ev[e++], s));
    bool near_live = false, overlap = false, rad = false;
    for (auto &cc : c.cia) overlap = overlap || cc.grid.max_overlap > CS_CIA_ACT;
    const FluxPlan pl = flux_plan(ctx->set, {c.nnu, c.np, c.nlob, c.K, c.nstream, !c.tab.empty(), !c.gas.empty(), overlap, ctx->gfx950, c.want_tau}, 1, &c.flux);
    FluxFuse fuse;
    memset(&fuse, 0, sizeof fuse);
    if ((rc = sigma_impl(ctx, s, ev, e, &log, &near_live, pl.form ? &fuse : nullptr, &pl))) return rc;
    c.near_live = near_live;
    c.sigma_partial = pl.form != 0;
    c.flux_last = pl;
    log.disp.flags |= pl.flags;
    if (ev) HIPCHK(hipEventRecord(ev[e++], s));
    const FluxArgs fa = {&c.rt, c.nu.as<double>(), c.wts.as<double>(), c.nnu, sig, c.muk.as<double>(), c.P.as<double>(), c.Tlev.as<double>(),
                         c.has_S ? c.S_toa.as<double>() : nullptr, c.has_alb ? c.albedo.as<double>() : nullptr,
                         c.want_tau == CS_TAU_LAYERS || pl.need_tau ? c.tau.as<double>() : nullptr, c.want_M ? c.Mup.as<double>() : nullptr, c.want_M ? c.Mdn.as<double>() : nullptr,
                         c.partial.as<double>(), s};
    const double *sigma2 = near_live ? c.sigma2.as<double>() : nullptr;
    if (pl.form) {
        fuse.sigma2 = sigma2; fuse.F = c.flux_out();
        fuse.ticket = pl.band_sum ? c.ticket.as<unsigned>() : nullptr;
        fuse.gpartial = c.partial.as<double>() + pl.gpartial * 2 * c.np;
        if (ctx->set.scan_stamps && c.fluxdbg.reserve((8 + 2 * (size_t)pl.nblk + 32) * sizeof(unsigned long long)) == hipSuccess) fuse.dbg = c.fluxdbg.as<unsigned long long>();
        for (int t = 0; t < fuse.ncia; t++) rad = rad || fuse.cia[t].Tr != nullptr;
    }
    if ((rc = launch_flux(pl, 1, fa, 0, sigma2, &fuse, rad))) return rc;
    if (ev) HIPCHK(hipEventRecord(ev[e++], s));
    if (pl.nfreduce) CS_LAUNCH(k_freduce, dim3(2 * c.np), dim3(256), 0, s, c.partial.as<double>(), pl.nfreduce, 2 * c.np, c.flux_out());
    if (ev) HIPCHK(hipEventRecord(ev[e++], s));
    if (c.depth_mode()) launch_depth(c, s, sigma2);   // (form 0: sig is finished, the near-line pairs in it or beside it)
    c.launches = g_nlaunch;
    c.log_last = log;
    HIPCHK(hipGetLastError());
    return CS_OK;
}

int cs_column_sigma_run(cs_ctx *ctx, void *stream)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    HIPCHK(hipSetDevice(ctx->device));
    int e = 0;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    const int rc = sigma_impl(ctx, s, nullptr, e, nullptr);
    if (rc) return rc;
    Column &c = ctx->col;
    if (c.depth_mode()) {   // the depths of the plane this call completed (near-line pairs folded in, clamped where a pedestal came off)
        launch_depth(c, s, nullptr);
        c.last_stream = s;
        HIPCHK(hipGetLastError());
    }
    return CS_OK;
}

int cs_column_run(cs_ctx *ctx, void *stream)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    HIPCHK(hipSetDevice(ctx->device));   // (a process may drive several contexts on several devices: cs_fluxes_discretized_multi)
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    Column &c = ctx->col;
    if (!ctx->set.graph) return run_impl(ctx, s, nullptr);
    if (c.graph_exec && c.has_phco2 && ctx->ph.builds != c.graph_ph_builds) drop_graph(c);   // (the captured launches name another layout of the levels)
    if (c.graph_exec) {
        {   // (a replayed graph carries the kernel arguments of the slots' old contents: gas tables, opacity tables, knots)
            const int rc0 = column_current(ctx);
            if (rc0) { drop_graph(c); return rc0; }
        }
        HIPCHK(hipGraphLaunch(c.graph_exec, s));
        // the replayed kernels wrote the near-line plane again and ran on THIS stream: what cs_column_sigma_fetch / cs_column_fetch /
        // cs_column_info read must say so, as after an eager run
        c.near_live = c.graph_near_live;
        c.sigma_partial = c.graph_sigma_partial;
        c.launches = c.graph_launches;
        c.log_last = c.graph_log;
        c.last_stream = s;
        return CS_OK;
    }
    if (c.runs_since_change++ == 0) return run_impl(ctx, s, nullptr);   // first run after a change: eager (workspaces may still grow)
    HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
    const int rc = run_impl(ctx, s, nullptr);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (rc || e != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        c.runs_since_change = 0;
        if (rc) return rc;
        return run_impl(ctx, s, nullptr);   // (capture refused: run eagerly)
    }
    c.graph = g;
    c.graph_near_live = c.near_live;   // (set by the captured run_impl)
    c.graph_sigma_partial = c.sigma_partial;
    c.graph_launches = c.launches;
    c.graph_log = c.log_last;
    c.graph_ph_builds = ctx->ph.builds;
    if (hipGraphInstantiate(&c.graph_exec, g, nullptr, nullptr, 0) != hipSuccess) { c.graph_exec = nullptr; drop_graph(c); return run_impl(ctx, s, nullptr); }
    HIPCHK(hipGraphLaunch(c.graph_exec, s));
    return CS_OK;
}

int cs_column_profile(cs_ctx *ctx, void *stream, int reps, double *ms)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "cs_column_setup has not been called");
    if (reps < 1 || !ms) return fail(CS_EINVAL, "bad arguments");
    Column &c = ctx->col;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    HIPCHK(hipSetDevice(ctx->device));
    const int ngrp = (int)c.gas.size();
    const int nev = 7 * ngrp + 4;
    std::vector<hipEvent_t> ev(nev);
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    for (int i = 0; i < 10; i++) ms[i] = 0.0;
    int rc = CS_OK;
    for (int r = 0; r < reps && rc == CS_OK; r++) {
        rc = run_impl(ctx, s, ev.data());
        if (rc) break;
        if (hipStreamSynchronize(s) != hipSuccess) { rc = fail(CS_EHIP, "hipStreamSynchronize failed"); break; }
        float t;
        const int slot[7] = {0, 1, 7, 3, 9, 8, 4};   // per gas: K1 + zones, nodes, nodes on the matrix cores, far, sub-tile cores, far on the matrix cores, near
        for (int gi = 0; gi < ngrp; gi++)
            for (int q = 0; q < 7; q++) { (void)hipEventElapsedTime(&t, ev[7 * gi + q], ev[7 * gi + q + 1]); ms[slot[q]] += t; }
        const int b = 7 * ngrp;
        (void)hipEventElapsedTime(&t, ev[b], ev[b + 1]); ms[2] += t;       // apply (+ baked tables, CIA)
        (void)hipEventElapsedTime(&t, ev[b + 1], ev[b + 2]); ms[5] += t;   // rt
        (void)hipEventElapsedTime(&t, ev[b + 2], ev[b + 3]); ms[6] += t;   // reduce
    }
    for (auto &e : ev) (void)hipEventDestroy(e);
    for (int i = 0; i < 10; i++) ms[i] /= reps;
    return rc;
}

int cs_column_sync(cs_ctx *ctx)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    return CS_OK;
}

int cs_column_flux_ptr(cs_ctx *ctx, double **dF)
{
    if (!ctx || !ctx->col.ready || !dF) return fail(CS_ESTATE, "no resident column");
    *dF = ctx->col.flux_out();
    return CS_OK;
}

int cs_column_flux_to(cs_ctx *ctx, double *dst_device, void *stream)
{
    if (!ctx || !ctx->col.ready || !dst_device) return fail(CS_ESTATE, "no resident column");
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    if (dst_device != ctx->col.flux_out())   // (the kernels write there already: cs_column_set_flux_dst)
        HIPCHK(hipMemcpyAsync(dst_device, ctx->col.flux_out(), (size_t)2 * ctx->col.np * sizeof(double), hipMemcpyDeviceToDevice, s));
    return CS_OK;
}

int cs_column_set_flux_dst(cs_ctx *ctx, double *dst_device)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "no resident column");
    if (ctx->col.F_dst != dst_device) drop_graph(ctx->col);   // (a captured step carries the old pointer)
    ctx->col.F_dst = dst_device;
    return CS_OK;
}

static int fetch_transposed(cs_ctx *ctx, const double *dsrc, int R, int64_t Cn, double *hdst)
{
    Column &c = ctx->col;
    hipStream_t s = ctx->stream;
    HIPCHK(c.stage.reserve((size_t)R * Cn * sizeof(double)));
    dim3 grid((unsigned)((Cn + 31) / 32), (unsigned)((R + 31) / 32));
    CS_LAUNCH(k_transpose, grid, dim3(256), 0, s, dsrc, R, Cn, c.stage.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(hdst, c.stage.p, (size_t)R * Cn * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CS_OK;
}

int cs_column_fetch(cs_ctx *ctx, int64_t nnu, int np, double *tau, double *Mup, double *Mdn, double *Fup, double *Fdn)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "no resident column");
    Column &c = ctx->col;
    if (nnu != c.nnu || np != c.np)   // the caller's buffers were sized for another column: refuse rather than overrun them
        return fail(CS_ESTATE, "resident column is %lld wavenumbers x %d levels, caller expects %lld x %d (another column was set up on this context)",
                    (long long)c.nnu, c.np, (long long)nnu, np);
    HIPCHK(hipSetDevice(ctx->device));
    // wait for the column's own work only (its run's stream; the side stream has been joined into it): other contexts on the same
    // device -- cs_fluxes_discretized_multi with several ranges per card -- keep computing while this one copies back
    if (c.last_stream && c.last_stream != ctx->stream) HIPCHK(hipStreamSynchronize(c.last_stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int rc;
    if (tau && !c.want_tau) return fail(CS_ESTATE, "column was set up without want_tau");
    // by the column's mode: [np - 1, nnu] layer depths, [nnu] slant depths of the whole column or [np, ntile] tile transmittances
    if (tau && c.want_tau == CS_TAU_LAYERS && (rc = fetch_transposed(ctx, c.tau.as<double>(), c.nl, c.nnu, tau))) return rc;
    if (tau && c.want_tau == CS_TAU_TOTAL) HIPCHK(hipMemcpyAsync(tau, c.depth.p, (size_t)c.nnu * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (tau && c.want_tau == CS_TAU_TILES && (rc = fetch_transposed(ctx, c.depth.as<double>(), c.np, c.m_ntile(), tau))) return rc;
    if ((Mup || Mdn) && !c.want_M) return fail(CS_ESTATE, "column was set up without want_M");
    // by the column's mode: [np, nnu] planes, [2, nnu] boundary spectra or [np, ntile] tile sums, column-major (level fastest) all three
    if (Mup && (rc = fetch_transposed(ctx, c.Mup.as<double>(), c.m_rows(), c.m_cols(), Mup))) return rc;
    if (Mdn && (rc = fetch_transposed(ctx, c.Mdn.as<double>(), c.m_rows(), c.m_cols(), Mdn))) return rc;
    if (Fup) HIPCHK(hipMemcpyAsync(Fup, c.flux_out(), c.np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (Fdn) HIPCHK(hipMemcpyAsync(Fdn, c.flux_out() + c.np, c.np * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

int cs_column_sigma_fetch(cs_ctx *ctx, int64_t nnu, int K, double *sigma)
{
    if (!ctx || !ctx->col.ready || !sigma) return fail(CS_ESTATE, "no resident column");
    Column &c = ctx->col;
    if (nnu != c.nnu || K != c.K)
        return fail(CS_ESTATE, "resident column is %lld wavenumbers x %d node states, caller expects %lld x %d", (long long)c.nnu, c.K,
                    (long long)nnu, K);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    if (c.sigma_partial) {   // the run finished the cross-sections on chip (k_flux): evaluate them once more, all the way into HBM
        int e = 0;
        const int rc = sigma_impl(ctx, ctx->stream, nullptr, e, nullptr);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(ctx->stream));
        c.sigma_partial = false;
        c.near_live = false;
    }
    if (c.near_live) {   // the run handed k_rt two planes: the total is their sum (folded in once)
        const int64_t tot = (int64_t)c.K * c.nnu;
        CS_LAUNCH(k_fold, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, tot, c.sigma.as<double>(), c.sigma2.as<double>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        c.near_live = false;
    }
    HIPCHK(hipMemcpy(sigma, c.sigma.p, (size_t)c.K * c.nnu * sizeof(double), hipMemcpyDeviceToHost));
    return CS_OK;
}

int cs_column_counts(cs_ctx *ctx, int64_t *pair_evals, int64_t *lines_in_range)
{
    if (!ctx || !ctx->col.ready) return fail(CS_ESTATE, "no resident column");
    Column &c = ctx->col;
    int64_t p = 0, l = 0;
    for (auto &g : c.ugas) {
        l += g.lines_in_range;
        if (shape_spec(g.shape).pshift) {   // (the flag, or code 7) pairs inside the cut-off of the shifted centres, state by state
            if (g.pairs_all < 0) {
                const GasTable &G = ctx->gas[g.slot];
                std::vector<double> sh(G.h_nu.size());
                g.pairs_all = 0;
                for (int k = 0; k < c.K; k++) {
                    for (size_t j = 0; j < sh.size(); j++) sh[j] = G.h_nu[j] + G.h_da[j] * c.h_Pk[k] / kAtm;
                    std::sort(sh.begin(), sh.end());
                    g.pairs_all += count_pairs(sh, c.h_nu.data(), c.nnu, g.cut);
                }
            }
            p += g.pairs_all;
            continue;
        }
        if (g.pairs_per_state < 0) g.pairs_per_state = count_pairs(ctx->gas[g.slot].h_nu, c.h_nu.data(), c.nnu, g.cut);
        p += g.pairs_per_state * c.K;
    }
    if (pair_evals) *pair_evals = p;
    if (lines_in_range) *lines_in_range = l;
    return CS_OK;
}

int cs_column_info(cs_ctx *ctx, int64_t *out)
{
    if (!ctx || !ctx->col.ready || !out) return fail(CS_ESTATE, "no resident column");
    const Column &c = ctx->col;
    for (int i = 0; i < 8; i++) out[i] = 0;
    out[0] = (int64_t)c.gas.size();
    out[1] = c.launches;
    for (auto &g : c.gas) { out[2] += g.tab->L; out[4] = std::max<int64_t>(out[4], (int64_t)g.mem.size()); }
    out[3] = c.merge;
    out[5] = c.flux_last.form;
    out[6] = c.log_last.near_launches;
    out[7] = c.log_last.line_kernel;
    return CS_OK;
}

int cs_interp_plan(int64_t nnu, const double *nu, double dnu_cut, int *interval_sizes)
{
    if (!nu || nnu < 1 || !interval_sizes) return fail(CS_EINVAL, "bad arguments");
    return choose_levels(nu, nnu, dnu_cut, interval_sizes);   // (default size range; a context's cs_set_interp_plan may narrow it)
}

// the virtual levels of a PhLevelSet as cs_phco2_plan reports them: (interval size, nodes, region mask) of the first `cap`; returns their number
static int ph_levels_out(const PhLevelSet &g, int cap, int *interval_sizes, int *nodes, int *regions)
{
    for (int v = 0; v < std::min(g.vl.nv, cap); v++) {
        interval_sizes[v] = g.lv.itv[g.vl.rl[v]];
        nodes[v] = g.vl.nc[v];
        regions[v] = g.vl.rmask[v];
    }
    return g.vl.nv;
}
int cs_phco2_plan(int64_t nnu, const double *nu, double dnu_cut, int cap, int *interval_sizes, int *nodes, int *regions)
{
    if (!nu || nnu < 1 || !interval_sizes || !nodes || !regions || cap < 1) return fail(CS_EINVAL, "bad arguments");
    return ph_levels_out(ph_levels(ph_grid(nu, nnu, 1), PhRules(), dnu_cut, 0), cap, interval_sizes, nodes, regions);
}

// test hooks: the plan under a context's settings (interpolation on / off, size range, margin, CS_TUNE_PH_NODES) with the regions of
// `drop` (bit r = region r + 1) kept out, and the mask ph_wide_regions forms from K states (T, Lorentz-width bound)
int cs_phco2_plan_ctx(cs_ctx *ctx, int64_t nnu, const double *nu, double dnu_cut, int drop, int cap, int *interval_sizes, int *nodes, int *regions)
{
    if (!ctx || !nu || nnu < 1 || !interval_sizes || !nodes || !regions || cap < 1 || drop < 0 || drop > 7) return fail(CS_EINVAL, "bad arguments");
    return ph_levels_out(ph_levels(ph_grid(nu, nnu, 1), ph_rules(*ctx), dnu_cut, drop), cap, interval_sizes, nodes, regions);
}
int cs_phco2_wide_regions(int K, const double *T, const double *gamma_bound, double dnu_cut)
{
    if (!T || !gamma_bound || K < 1) return fail(CS_EINVAL, "bad arguments");
    return ph_wide_regions(T, gamma_bound, K, dnu_cut);
}

// ---- cs_column_work: one routine per kernel family.  Each counts one Voigt / Lorentz group of the column from the tables its last run
// left on the device (WorkTables, downloaded once per group) and from the plan that run was dispatched by (ColGas::plan) -- never from
// the context's settings, which may have changed since.
struct WorkTables {
    std::vector<WaveWin> win;   // [tiles]
    std::vector<Zone> zn;       // [K][tiles]
    std::vector<IZone> iz;      // [K][nItot] (interpolated wings)
    std::vector<SepZone> sz;    // [K/16][nItot] (plan.use_sep)
    std::vector<EdgeZone> ez;   // [K/16][tiles] (plan.use_edge)
};
struct Work {
    int64_t direct = 0, nodes = 0;
    int64_t sepn = 0, edgen = 0;   // (node | point, line, state) triples summed on the matrix cores; mx3, mx3n: those (of sepn) with 3 terms; mx8: with 8
    int64_t mx3 = 0, mx3n = 0, mx8 = 0;
    int64_t subn = 0, subn_lean = 0, ncore = 0;   // (lane, line) evaluations of k_voigt_sub, those of waves that start range-only; (tile, state) cores
    // flops of the two matrix-core kernels: issued = every matrix instruction's 2048; useful = 2 x terms per (column, line, state) with
    // the column inside the cut-off, outside the core radius, and the state a real one (a group's tail rows are padding)
    double fl_edge_useful = 0.0, fl_edge_issued = 0.0, fl_nodes_useful = 0.0, fl_nodes_issued = 0.0, fl_apply = 0.0;
    int64_t rec_edge = 0, rec_nodes = 0;   // (state, line) records the two matrix-core kernels REQUEST: lines of every piece x 16 states (neighbouring tiles and
                                           // intervals ask for the same record again: the unique ones are K x lines in range)
    int64_t near0 = 0, near1 = 0;
    int64_t body[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // per-point lines by body: 2-term, 2-term+cut-off, 3-term, 3-term+cut-off, 4-term+cut-off,
                                                     // near-zone pass; node lines: 2-, 3-, 4-term
};
static int64_t work_seg(int lo, int hi, int p0, int p1) { return (int64_t)std::max(0, std::min(hi, p1) - std::max(lo, p0)); }

// node sums: k_cheb_nodes on the vector unit, k_cheb_nodes_mx on the matrix cores (useful flops per state, issued and records per group)
static void work_nodes(const Column &c, const ColGas &g, const WorkTables &T, Work &w)
{
    const VoigtPlan &pl = g.plan;
    const int K = c.K, nlev = g.itp.nlev, nItot = c.cheb.nItot, q0 = pl.q0;
    // nodes a piece of interval q is summed on in k_cheb_nodes_mx: its level's 16 or 32 for the far pieces (p = 0, 3) where the
    // re-interpolation matrices are in use, 64 otherwise (the carry to the 64 nodes, 2 x 64 x n per state, is not counted)
    auto far_nodes = [&](int q, int p) {
        if (!pl.far_R || (p != 0 && p != 3)) return (int)CS_NC;
        int l = 0;
        while (l + 1 < nlev && q >= c.cheb.ioff[l + 1]) l++;
        return pl.nfar[l];
    };
    for (int k = 0; k < K; k++)
        for (int q = q0; q < nItot; q++) {
            const IZone &z = T.iz[(size_t)k * nItot + q];
            w.nodes += (int64_t)CS_NC * ((z.P0 - z.E0) + (z.Z0 - z.P1) + (z.P2 - z.Z1) + (z.E1 - z.P3));
            // the same segments k_cheb_nodes runs: [E0,P0) U [P1,Z0) left, [Z1,P2) U [P3,E1) right, each minus the piece
            // the matrix-core kernel takes, cut at Q and M
            int sa[4] = {z.P0, z.Z0, z.Z1, z.P3}, sb[4] = {z.P0, z.Z0, z.Z1, z.P3};
            if (pl.use_sep) {
                const SepZone &s4 = T.sz[(size_t)(k >> 4) * nItot + q];
                for (int p = 0; p < 4; p++) {   // of the group's piece, this state's part: the lines beyond its own series radius (k_cheb_nodes_mx's mask)
                    const SepShare sh = sep_share(s4, p, z);
                    const int pa = sh.a, pb = sh.b;
                    if (pb > pa) {
                        sa[p] = pa; sb[p] = pb; w.sepn += (int64_t)CS_NC * (pb - pa);
                        const int n3 = p < 2 ? std::max(0, std::min(s4.m[p], pb) - pa) : std::max(0, pb - std::max(s4.m[p], pa));
                        w.mx3 += (int64_t)CS_NC * n3;
                        w.mx3n += (int64_t)CS_NC * n3;
                        w.fl_nodes_useful += 2.0 * far_nodes(q, p) * (3.0 * n3 + 4.0 * ((pb - pa) - n3));
                    }
                }
            }
            const int lo8[8] = {z.E0, sb[0], z.P1, sb[1], sb[3], z.P3, sb[2], z.Z1}, hi8[8] = {sa[0], z.P0, sa[1], z.Z0, z.E1, sa[3], z.P2, sa[2]};
            for (int w8 = 0; w8 < 8; w8++) {
                const int p0 = lo8[w8], p1 = hi8[w8];
                if (w8 < 4) {
                    w.body[6] += work_seg(z.E0, z.Q0, p0, p1); w.body[7] += work_seg(z.Q0, z.M0, p0, p1); w.body[8] += work_seg(z.M0, z.Z0, p0, p1);
                } else {
                    w.body[6] += work_seg(z.Q1, z.E1, p0, p1); w.body[7] += work_seg(z.M1, z.Q1, p0, p1); w.body[8] += work_seg(z.Z1, z.M1, p0, p1);
                }
            }
        }
    if (!pl.use_sep) return;
    for (int gq = 0; gq < pl.ngrp; gq++)
        for (int q = q0; q < nItot; q++) {
            const SepZone &z = T.sz[(size_t)gq * nItot + q];
            for (int p = 0; p < 4; p++) {
                if (z.b[p] <= z.a[p]) continue;
                const int n3 = p < 2 ? z.m[p] - z.a[p] : z.b[p] - z.m[p], n4 = (z.b[p] - z.a[p]) - n3;
                w.rec_nodes += 16 * (int64_t)(n3 + n4);
                w.fl_nodes_issued += 2.0 * far_nodes(q, p) * 16 * (3.0 * ((n3 + 3) / 4 * 4) + 4.0 * ((n4 + 3) / 4 * 4));
            }
        }
}

// the pieces of k_voigt_edge_mx per (tile, state group): records requested and flops
static void work_edge(const Column &c, const ColGas &g, const WorkTables &T, Work &w)
{
    const VoigtPlan &pl = g.plan;
    const int K = c.K, nt64 = pl.nt64;
    const double *nl = g.tab->h_nu.data(), *vv = c.h_nu.data();
    // the cut-off edges, cut where the next sub-tile comes into reach (k_voigt_edge_mx's phases: one wave per (tile, group) only)
    const bool phased = pl.edge_phases && pl.edge_big;
    for (int gq = 0; gq < pl.ngrp; gq++) {
        const int ns = std::min(16, K - 16 * gq);
        for (int t = 0; t < nt64; t++) {
            const WaveWin win = T.win[t];
            const EdgeZone e = T.ez[(size_t)gq * nt64 + t];
            const double *v0 = vv + (size_t)t * 64, *v1 = vv + std::min<int64_t>((int64_t)t * 64 + 64, c.nnu);
            auto piece = [&](int ja, int jb, int nt, int mask) {   // mask 1: the points with |dnu| <= cut count; 2: also |dnu| >= R
                if (jb <= ja) return;
                w.rec_edge += 16 * (int64_t)(jb - ja);
                w.fl_edge_issued += 2.0 * nt * 64.0 * 16.0 * ((jb - ja + 3) / 4 * 4);
                double cols = 0.0;
                for (int j = ja; j < jb; j++) {
                    int n = (int)(std::upper_bound(v0, v1, nl[j] + g.cut) - std::lower_bound(v0, v1, nl[j] - g.cut));
                    if (mask == 2) n -= (int)(std::lower_bound(v0, v1, nl[j] + e.R) - std::upper_bound(v0, v1, nl[j] - e.R));   // (|dnu| < R: k_voigt_sub's)
                    cols += std::max(n, 0);
                }
                w.fl_edge_useful += 2.0 * nt * cols * ns;
            };
            bool tile_carry = false;
            // a window end: the lines [ja, jb) left or right of the tile
            auto end_piece = [&](int ja, int jb, int nt, bool left) {
                if (jb <= ja) return;
                if (!phased || jb - ja < 48) { piece(ja, jb, nt, 1); return; }
                const double issued0 = w.fl_edge_issued;
                piece(ja, jb, nt, 1);              // (for the useful flops)
                w.fl_edge_issued = issued0;
                const double tolc = 1e-9 * (std::fabs(v0[0]) + g.cut + 1.0);
                // the lines inside the cut-off of every point of the tile (those nearest to it): on 16 nodes of the tile (one sub-tile
                // per step) + the carry to the points, 16 matrix instructions per (tile, group) that has any
                if (pl.tnodes) {
                    const int jt = (int)((left ? std::lower_bound(nl + ja, nl + jb, *(v1 - 1) - g.cut + tolc)
                                               : std::upper_bound(nl + ja, nl + jb, v0[0] + g.cut - tolc)) - nl);
                    const int nin = left ? jb - jt : jt - ja;
                    if (nin >= 16) {
                        w.fl_edge_issued += 2.0 * nt * 16.0 * 16.0 * ((nin + 3) / 4 * 4);
                        tile_carry = true;
                        (left ? jb : ja) = jt;
                    }
                }
                // the rest in four parts: part q reaches q + 1 (left) | 4 - q (right) of the tile's four sub-tiles
                int cutp[5];
                cutp[0] = ja; cutp[4] = jb;
                for (int q = 0; q < 3; q++) {
                    const double col = vv[std::min<int64_t>((int64_t)t * 64 + (left ? 16 * (q + 1) : 16 * q + 15), c.nnu - 1)];
                    cutp[q + 1] = (int)((left ? std::lower_bound(nl + ja, nl + jb, col - g.cut - tolc)
                                              : std::upper_bound(nl + ja, nl + jb, col + g.cut + tolc)) - nl);
                }
                for (int q = 1; q < 5; q++) cutp[q] = std::max(cutp[q], cutp[q - 1]);
                for (int q = 0; q < 4; q++) w.fl_edge_issued += 2.0 * nt * 16.0 * (left ? q + 1 : 4 - q) * 16.0 * ((cutp[q + 1] - cutp[q] + 3) / 4 * 4);
            };
            end_piece(win.W0, e.eL, (e.far3 & 1) ? 3 : 4, true);
            end_piece(e.eR, win.W1, (e.far3 & 2) ? 3 : 4, false);
            if (tile_carry) w.fl_edge_issued += 16.0 * 2048.0;
            if (e.mL1 > e.mL0) { piece(e.mL0, e.mL3, 3, 1); piece(e.mL3, e.mL1, 4, 1); }
            if (e.mR1 > e.mR0) { piece(e.mR3, e.mR1, 3, 1); piece(e.mR0, e.mR3, 4, 1); }
            if (e.cR > e.cL) piece(e.cL, e.cR, (e.far3 & 4) ? 8 : 4, 2);
        }
    }
}

// per (tile, state): the direct bodies of k_voigt_far, what k_voigt_edge_mx takes of the window instead, and k_voigt_sub
static void work_direct(const Column &c, const ColGas &g, const WorkTables &T, Work &w)
{
    const VoigtPlan &pl = g.plan;
    const int K = c.K, nt64 = pl.nt64, nlev = g.itp.nlev, nItot = c.cheb.nItot;
    const double *nl = g.tab->h_nu.data();
    for (int k = 0; k < K; k++)
        for (int t = 0; t < nt64; t++) {
            WaveWin win = T.win[t];
            const Zone &z = T.zn[(size_t)k * nt64 + t];
            const int W0 = win.W0, W1 = win.W1;
            int pm[4] = {0, 0, 0, 0};   // [pL0, pL1), [pR0, pR1): the pieces between interpolated sets and near zone on the matrix cores
            int cc0 = 0, cc1 = 0;       // [cc0, cc1): the core that k_voigt_sub and the second mask of k_voigt_edge_mx share
            if (pl.use_edge) {   // what k_voigt_edge_mx takes
                const EdgeZone e = T.ez[(size_t)(k >> 4) * nt64 + t];
                w.edgen += 64 * (int64_t)((e.eL - W0) + (W1 - e.eR));
                w.mx3 += 64 * (int64_t)(((e.far3 & 1) ? e.eL - W0 : 0) + ((e.far3 & 2) ? W1 - e.eR : 0));
                win.W0 = e.eL; win.W1 = e.eR;
                if (e.mL1 > e.mL0) { pm[0] = e.mL0; pm[1] = e.mL1; w.mx3 += 64 * (int64_t)(e.mL3 - e.mL0); }
                if (e.mR1 > e.mR0) { pm[2] = e.mR0; pm[3] = e.mR1; w.mx3 += 64 * (int64_t)(e.mR1 - e.mR3); }
                w.edgen += 64 * (int64_t)((pm[1] - pm[0]) + (pm[3] - pm[2]));
                if (e.cR > e.cL) {   // the core: every pair visits the matrix cores (masked inside R), k_voigt_sub the lines within R of each sub-tile
                    cc0 = e.cL; cc1 = e.cR;
                    w.ncore++;
                    w.edgen += 64 * (int64_t)(e.cR - e.cL);
                    if (e.far3 & 4) w.mx8 += 64 * (int64_t)(e.cR - e.cL);
                    for (int q4 = 0; q4 < 64 / CS_SUBW; q4++) {   // (k_voigt_sub<CS_SUBW>)
                        const double v0 = c.h_nu[(size_t)t * 64 + CS_SUBW * q4] - e.R, v1 = c.h_nu[(size_t)t * 64 + CS_SUBW * q4 + CS_SUBW - 1] + e.R;
                        const int ja = (int)(std::lower_bound(nl + e.cL, nl + e.cR, v0) - nl);
                        const int jb = (int)(std::upper_bound(nl + ja, nl + e.cR, v1) - nl);
                        w.subn += CS_SUBW * (int64_t)(jb - ja);
                        if (pl.sub_lean != 1 && ((e.lean >> ((k >> 3) & 1)) & 1)) w.subn_lean += CS_SUBW * (int64_t)(jb - ja);
                    }
                }
            }
            int64_t n = (win.W1 - win.W0) - (pm[1] - pm[0]) - (pm[3] - pm[2]) - (cc1 - cc0);
            const FarCovered fc = nlev > 0 ? far_covered(z, T.iz[(size_t)k * nItot + c.cheb.ioff[nlev - 1] + (t >> pl.ishift)], T.win[t]) : far_covered(z);
            const int sa0 = fc.sa0, sa1 = fc.sa1, sb0 = fc.sb0, sb1 = fc.sb1;
            n -= (sa1 - sa0) + (sb1 - sb0);   // (both empty without interpolated wings)
            w.direct += 64 * n;
            // the same segments k_voigt_far runs inside its three clip windows
            const int a = std::min(std::max(win.E0, W0), z.Q0), a1 = std::min(std::max(win.E0, z.Q0), z.M0);
            const int b1 = std::max(std::min(win.E1, z.Q1), z.M1), bq = std::max(std::min(win.E1, W1), z.Q1);
            const int pL0 = pm[1] > pm[0] ? pm[0] : sa1, pL1 = pm[1] > pm[0] ? pm[1] : sa1;
            const int pR0 = pm[3] > pm[2] ? pm[2] : sb0, pR1 = pm[3] > pm[2] ? pm[3] : sb0;
            const int cM0 = cc1 > cc0 ? cc0 : pR0, cM1 = cc1 > cc0 ? cc1 : pR0;
            const int cl[6] = {win.W0, sa1, pL1, cM1, pR1, sb1}, ch[6] = {sa0, pL0, cM0, pR0, sb0, win.W1};
            for (int cw = 0; cw < 6; cw++) {
                const int p0 = cl[cw], p1 = ch[cw];
                if (p0 >= p1) continue;
                w.body[1] += work_seg(W0, a, p0, p1) + work_seg(bq, W1, p0, p1);
                w.body[0] += work_seg(a, z.Q0, p0, p1) + work_seg(z.Q1, bq, p0, p1);
                w.body[3] += work_seg(z.Q0, a1, p0, p1) + work_seg(b1, z.Q1, p0, p1);
                w.body[2] += work_seg(a1, z.M0, p0, p1) + work_seg(z.M1, b1, p0, p1);
                w.body[4] += work_seg(z.M0, z.N0, p0, p1) + work_seg(z.N1, z.M1, p0, p1);
                w.body[5] += work_seg(z.N0, z.N1, p0, p1);
            }
        }
}

// near-line pairs by tier (k_voigt_near<0>: 100 <= s < 1e3, <1>: s < 100), counted from the records of the launch group whose
// per-(state, line) records are still in HBM -- the last Voigt group of the column (the only one when its gases are merged)
static int work_near(const Column &c, Work &w)
{
    if (c.gas.empty() || c.gas.back().shape != SH_VOIGT || c.gas.back().w.jhi <= c.gas.back().w.jlo) return CS_OK;
    const ColGas &g = c.gas.back();
    const int64_t L = g.tab->L, nj = g.w.jhi - g.w.jlo;
    std::vector<LineHot> rec((size_t)nj);
    const double *vv = c.h_nu.data();
    const int64_t nnu = c.nnu;
    for (int k = 0; k < c.K; k++) {
        HIPCHK(hipMemcpy(rec.data(), c.hot.as<LineHot>() + (size_t)k * L + g.w.jlo, rec.size() * sizeof(LineHot), hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < nj; j++) {
            const LineHot &h = rec[j];
            auto within = [&](double smax) -> int64_t {   // points with x^2 + y^2 < smax and |dnu| <= cut
                if (!(h.p2 < smax)) return 0;
                const double r = std::min(std::sqrt(smax - h.p2) / h.p1, g.cut);
                return (std::lower_bound(vv, vv + nnu, h.nul + r) - std::upper_bound(vv, vv + nnu, h.nul - r));
            };
            const int64_t n1 = within(kMidS), n0 = within(kSerS);
            w.near1 += n1;
            w.near0 += n0 - n1;
        }
    }
    return CS_OK;
}

int cs_column_work(cs_ctx *ctx, int64_t *out)
{
    if (!ctx || !ctx->col.ready || !out) return fail(CS_ESTATE, "no resident column");
    Column &c = ctx->col;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    const int K = c.K;
    int rc;
    Work w;
    auto download = [](auto &h, const DevBuf &d, size_t n) -> int {
        h.resize(n);
        HIPCHK(hipMemcpy(h.data(), d.p, n * sizeof h[0], hipMemcpyDeviceToHost));
        return CS_OK;
    };
    for (auto &g : c.gas) {
        // (a batch right after setup writes its windows and zones into buffers of its own: nothing to count, and the column's are unwritten)
        if (!g.planned) continue;
        const VoigtPlan &pl = g.plan;
        const int nlev = g.itp.nlev, nItot = c.cheb.nItot;
        WorkTables T;
        if ((rc = download(T.win, g.w.win, (size_t)pl.nt64)) || (rc = download(T.zn, g.zones, (size_t)K * pl.nt64)) ||
            (nlev > 0 && (rc = download(T.iz, g.itp.iz, (size_t)K * nItot))) ||
            (pl.use_sep && (rc = download(T.sz, g.itp.sep, (size_t)pl.ngrp * nItot))) ||
            (pl.use_edge && (rc = download(T.ez, g.itp.edge, (size_t)pl.ngrp * pl.nt64))))
            return rc;
        if (nlev > 0) work_nodes(c, g, T, w);
        if (pl.use_edge) work_edge(c, g, T, w);
        if (nlev > 0)   // the contraction that carries the node sums to the grid (k_cheb_apply_mfma, or fused into k_voigt_edge_mx)
            w.fl_apply += 2.0 * CS_NC * 64.0 * 16.0 * pl.ngrp * (double)pl.nt64 * (nlev - g.itp.l0);   // (per group; with the cascade: cs_column_info)
        work_direct(c, g, T, w);
    }
    if ((rc = work_near(c, w))) return rc;
    out[CS_WORK_DIRECT_EVALS] = w.direct;
    out[CS_WORK_NODE_EVALS] = w.nodes;
    out[CS_WORK_LEVELS] = c.cheb.nlev;
    out[CS_WORK_INTERVALS] = c.cheb.nItot;
    for (int q = 0; q < 6; q++) out[CS_WORK_DIRECT_T2 + q] = 64 * w.body[q];
    for (int q = 0; q < 3; q++) out[CS_WORK_NODE_T2 + q] = (int64_t)CS_NC * w.body[6 + q];
    out[CS_WORK_NODE_EVALS_MATRIX] = w.sepn;
    out[CS_WORK_DIRECT_EVALS_MATRIX] = w.edgen;
    out[CS_WORK_MATRIX_EVALS_3TERM] = w.mx3;
    out[CS_WORK_SUB_EVALS] = w.subn;
    out[CS_WORK_CORE_TILE_STATES] = w.ncore;
    out[CS_WORK_MATRIX_EVALS_8TERM] = w.mx8;
    out[CS_WORK_NODE_EVALS_MATRIX_3TERM] = w.mx3n;
    out[CS_WORK_NEAR_PAIRS_TIER0] = w.near0;
    out[CS_WORK_NEAR_PAIRS_TIER1] = w.near1;
    out[CS_WORK_EDGE_MX_FLOPS_USEFUL] = (int64_t)w.fl_edge_useful;
    out[CS_WORK_EDGE_MX_FLOPS_ISSUED] = (int64_t)w.fl_edge_issued;
    out[CS_WORK_NODES_MX_FLOPS_USEFUL] = (int64_t)w.fl_nodes_useful;
    out[CS_WORK_NODES_MX_FLOPS_ISSUED] = (int64_t)w.fl_nodes_issued;
    out[CS_WORK_APPLY_FLOPS] = (int64_t)w.fl_apply;
    out[CS_WORK_EDGE_MX_RECORD_BYTES] = w.rec_edge * (int64_t)sizeof(LineHot);
    out[CS_WORK_NODES_MX_RECORD_BYTES] = w.rec_nodes * (int64_t)sizeof(LineHot);
    out[CS_WORK_FAR_SPLIT] = c.log_last.disp.far_split;
    out[CS_WORK_TABLES] = c.log_last.disp.tables;
    out[CS_WORK_NEAR_PRIO] = c.log_last.disp.near_prio;
    out[CS_WORK_STREAMS] = c.log_last.disp.streams;
    out[CS_WORK_NODES_SPLIT] = c.log_last.disp.nodes_split;
    out[CS_WORK_FLAGS] = c.log_last.disp.flags;
    out[CS_WORK_SUB_LEAN_EVALS] = w.subn_lean;
    // (the flux-phase stamps describe the stamp buffer's contents: the only part that looks at a setting)
    if (c.fluxdbg.p && ctx->set.scan_stamps) {   // k_flux_scan's phases in block 0, ns: cross-sections, depths + Planck, chunk pass, hand-over, second pass, band sum
        unsigned long long st[8] = {};
        (void)hipMemcpy(st, c.fluxdbg.p, sizeof st, hipMemcpyDeviceToHost);
        for (int q = 0; q < 4; q++) out[CS_WORK_FLUX_SCAN_NS + q] = (int64_t)(st[q + 1] - st[q]) * 10;   // (100 MHz clock)
        out[CS_WORK_FLUX_SCAN_TOTAL_NS] = (int64_t)(st[7] - st[0]) * 10;   // block 0's first instruction to the last block's last word
        if (getenv("CS_FLUX_DBG") && c.flux_last.form == 3) {   // every block's start and end (k_flux_scan), relative to the earliest start
            const size_t nb = (size_t)c.flux_last.nblk;
            if (c.fluxdbg.bytes >= (8 + 2 * nb + 32) * sizeof(unsigned long long)) {
                std::vector<unsigned long long> bs(2 * nb + 32);
                (void)hipMemcpy(bs.data(), (const char *)c.fluxdbg.p + 8 * sizeof(unsigned long long), (2 * nb + 32) * sizeof(unsigned long long), hipMemcpyDeviceToHost);
                fprintf(stderr, "block 0 fine stamps [us from its start]: hand-over steps");
                for (int q = 0; q < 12; q++) fprintf(stderr, " %.1f", (double)(bs[2 * nb + q] - st[0]) * 0.01);
                fprintf(stderr, " | second pass down");
                for (int q = 0; q < 5; q++) fprintf(stderr, " %.1f", (double)(bs[2 * nb + 16 + q] - st[0]) * 0.01);
                fprintf(stderr, " up");
                for (int q = 4; q >= 0; q--) fprintf(stderr, " %.1f", (double)(bs[2 * nb + 24 + q] - st[0]) * 0.01);
                fprintf(stderr, "\n");
                unsigned long long t0 = ~0ull;
                for (size_t b = 0; b < nb; b++) t0 = std::min(t0, bs[2 * b]);
                std::vector<double> st0(nb), en0(nb), du(nb);
                for (size_t b = 0; b < nb; b++) { st0[b] = (double)(bs[2 * b] - t0) * 0.01; en0[b] = (double)(bs[2 * b + 1] - t0) * 0.01; du[b] = en0[b] - st0[b]; }
                auto pct = [](std::vector<double> v, double q) { std::sort(v.begin(), v.end()); return v[(size_t)(q * (double)(v.size() - 1))]; };
                fprintf(stderr, "block 0 stamps [us from its start]:");
                for (int q = 1; q < 7; q++) fprintf(stderr, " %.1f", (double)(st[q] - st[0]) * 0.01);
                fprintf(stderr, "\n");
                fprintf(stderr, "flux blocks %zu [us]: start p50 %.1f p90 %.1f max %.1f | duration min %.1f p50 %.1f p90 %.1f max %.1f | end p50 %.1f p90 %.1f max %.1f | band fluxes stored %.1f\n",
                        nb, pct(st0, 0.5), pct(st0, 0.9), pct(st0, 1.0), pct(du, 0.0), pct(du, 0.5), pct(du, 0.9), pct(du, 1.0), pct(en0, 0.5), pct(en0, 0.9), pct(en0, 1.0),
                        (double)(st[7] - t0) * 0.01);
            }
        }
    } else {
        for (int q = CS_WORK_FLUX_SCAN_NS; q <= CS_WORK_FLUX_SCAN_TOTAL_NS; q++) out[q] = 0;
    }
    return CS_OK;
}

// true when the resident column was set up for exactly this grid, pressure levels, rule orders and gas line-up: only the
// thermal state and the per-call spectra differ, so a call can skip the window / interpolation-matrix / workspace setup
// (the members beyond line-by-line gases -- baked tables, CIA pairs, an accelerated absorber -- are named by their slots: ntab / ncia
//  = 0 and accel_slot = -1 for a column without them)
static bool column_matches(cs_ctx *ctx, int64_t nnu, const double *nu, int np, const double *P, double g, int nlobatto, int ngas,
                           const int *gas_slots, const int *shapes, const double *dnu_cuts, double sigma_gray, double theta_s,
                           int nstream, int want_tau, int want_M, int64_t g_nnu = 0, int64_t g_start = 0, double g_left = 0.0, double g_right = 0.0,
                           int ntab = 0, const int *table_slots = nullptr, int ncia = 0, const int *cia_slots = nullptr, int accel_slot = -1)
{
    const Column &c = ctx->col;
    const bool shard_ok = g_nnu > 0 ? (!c.default_wts && c.g_nnu == g_nnu && c.g_start == g_start && c.g_left == g_left && c.g_right == g_right)
                                    : c.default_wts;
    if (!c.ready || c.accel.slot != accel_slot || !shard_ok || c.interp != interp_key(ctx) || (int)c.tab.size() != ntab || (int)c.cia.size() != ncia) return false;
    for (int t = 0; t < ntab; t++)
        if (c.tab[t].slot != table_slots[t]) return false;
    for (int t = 0; t < ncia; t++)
        if (c.cia[t].slot != cia_slots[t]) return false;
    if (c.nnu != nnu || c.np != np || c.nlob != nlobatto || c.nstream != nstream || c.ngas != ngas) return false;
    if (c.g != g || c.sigma_gray != sigma_gray || c.theta_s != theta_s) return false;
    if (c.want_tau != want_tau || c.want_M != want_M) return false;   // (modes compared: an edges or tiles column is no planes column -- its M buffers are smaller -- and a total or tiles column holds no layer depths)
    if (c.merge != ctx->merge) return false;
    for (int gi = 0; gi < ngas; gi++) {
        const UserGas &cg = c.ugas[gi];
        if (cg.slot != gas_slots[gi] || cg.shape != (shapes ? shapes[gi] : CS_SHAPE_VOIGT) || cg.cut != (dnu_cuts ? dnu_cuts[gi] : 25.0)) return false;
        if (gas_slots[gi] < 0 || gas_slots[gi] >= CS_MAX_GAS || !ctx->gas[cg.slot].present || ctx->gas[cg.slot].generation != cg.generation) return false;
    }
    return memcmp(c.h_nu.data(), nu, (size_t)nnu * sizeof(double)) == 0 && memcmp(c.h_P.data(), P, (size_t)np * sizeof(double)) == 0;
}

int cs_fluxes_discretized(cs_ctx *ctx, int64_t nnu, const double *nu, int np, const double *P, double g, int nlobatto,
                          const double *T_nodes, const double *mu_nodes, const double *T_levels, int ngas,
                          const int *gas_slots, const int *shapes, const double *dnu_cuts, const double *conc,
                          double sigma_gray, const double *sigma_extra, const double *S_toa, const double *albedo,
                          double theta_s, int nstream, double *tau, double *Mup, double *Mdn, double *Fup, double *Fdn)
{
    return cs_fluxes_discretized_members(ctx, nnu, nu, np, P, g, nlobatto, T_nodes, mu_nodes, T_levels, ngas, gas_slots, shapes, dnu_cuts, conc,
                                         0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, -1, sigma_gray, sigma_extra, S_toa, albedo,
                                         theta_s, nstream, tau, Mup, Mdn, Fup, Fdn);
}

int cs_fluxes_discretized_members(cs_ctx *ctx, int64_t nnu, const double *nu, int np, const double *P, double g, int nlobatto,
                                  const double *T_nodes, const double *mu_nodes, const double *T_levels, int ngas,
                                  const int *gas_slots, const int *shapes, const double *dnu_cuts, const double *conc,
                                  int ntab, const int *table_slots, const double *conc_tab,
                                  int ncia, const int *cia_slots, const int *cia_flags, const double *cia_P1, const double *cia_P2,
                                  int accel_slot, double sigma_gray, const double *sigma_extra, const double *S_toa, const double *albedo,
                                  double theta_s, int nstream, double *tau, double *Mup, double *Mdn, double *Fup, double *Fdn)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (!nu || !P || nnu < 1 || np < 2) return fail(CS_EINVAL, "bad grid arguments");
    if (ntab < 0 || ntab > CS_MAX_TABLE || (ntab > 0 && (!table_slots || !conc_tab))) return fail(CS_EINVAL, "bad opacity-table arguments");
    if (ncia < 0 || ncia > CS_MAX_CIA || (ncia > 0 && (!cia_slots || !cia_P1 || !cia_P2))) return fail(CS_EINVAL, "bad CIA arguments");
    if (accel_slot >= 0 && (ngas > 0 || ntab > 0 || ncia > 0))   // unifyabsorbers(::Tuple{AcceleratedAbsorber}), absorbers.jl:216
        return fail(CS_EINVAL, "a column over an accelerated absorber has no other absorbers");
    if (accel_slot < -1) accel_slot = -1;
    int rc;
    // radiate! is called once per time step / Jacobian column on an unchanged grid (radiative_convective.jl:109-171): keep the
    // column of the previous call resident and refresh only what a call can change -- node states, fS, fa, sigma_extra, and the
    // per-node inputs of the tables / CIA pairs / accelerated absorber it names
    if (column_matches(ctx, nnu, nu, np, P, g, nlobatto, ngas, gas_slots, shapes, dnu_cuts, sigma_gray, theta_s, nstream,
                       tau ? CS_TAU_LAYERS : CS_TAU_NONE, (Mup || Mdn) ? CS_M_PLANES : CS_M_NONE, 0, 0, 0.0, 0.0, ntab, table_slots, ncia, cia_slots, accel_slot)) {
        Column &c = ctx->col;
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        const bool was[3] = {c.has_extra, c.has_S, c.has_alb};
        c.has_extra = sigma_extra != nullptr;
        c.has_S = S_toa != nullptr && std::any_of(S_toa, S_toa + nnu, [](double x) { return x != 0.0; });
        c.has_alb = albedo != nullptr && std::any_of(albedo, albedo + nnu, [](double x) { return x != 0.0; });
        if (was[0] != c.has_extra || was[1] != c.has_S || was[2] != c.has_alb) drop_graph(c);   // (other kernel arguments)
        if (c.has_extra && (rc = upload(c.extra, sigma_extra, (size_t)nnu * c.K, s))) return rc;
        if (c.has_S && (rc = upload(c.S_toa, S_toa, nnu, s))) return rc;
        if (c.has_alb && (rc = upload(c.albedo, albedo, nnu, s))) return rc;
        // (a table baked again into its slot since the last call may have another (T, P) grid: cs_column_set_tables re-checks it)
        if (ntab > 0 && (rc = cs_column_set_tables(ctx, ntab, table_slots, conc_tab))) return rc;
        if ((rc = cs_column_update_state(ctx, T_nodes, mu_nodes, T_levels, conc, ntab > 0 ? conc_tab : nullptr))) return rc;
    } else {
        rc = cs_column_setup(ctx, nnu, nu, nullptr, np, P, g, nlobatto, T_nodes, mu_nodes, T_levels, ngas, gas_slots,
                             shapes, dnu_cuts, conc, sigma_gray, sigma_extra, S_toa, albedo, theta_s, nstream,
                             tau ? CS_TAU_LAYERS : CS_TAU_NONE, (Mup || Mdn) ? CS_M_PLANES : CS_M_NONE);
        if (rc) return rc;
        if (ntab > 0 && (rc = cs_column_set_tables(ctx, ntab, table_slots, conc_tab))) return rc;
    }
    // per-node partial pressures of the CIA pairs and the knot cells of the accelerated absorber follow the node states: every call
    if (ncia > 0 && (rc = cs_column_set_cia(ctx, ncia, cia_slots, cia_flags, cia_P1, cia_P2))) return rc;
    if (accel_slot >= 0 && (rc = cs_column_set_accel(ctx, accel_slot))) return rc;
    if ((rc = cs_column_run(ctx, nullptr))) return rc;
    return cs_column_fetch(ctx, nnu, np, tau, Mup, Mdn, Fup, Fdn);
}

// ---- host-held reference objects handed over as they are ---------------------------------------------------------------------
// x[0..n) = chebygrid(x[0], x[n-1], n) (Chebyshev extrema, ascending) to 1e-9 of the range
static bool cheb_extrema(const double *x, int n)
{
    const double a = x[0], b = x[n - 1];
    for (int i = 0; i < n; i++) {
        const double e = (std::cos(M_PI * (n - 1 - i) / (n - 1)) + 1.0) * (b - a) / 2.0 + a;
        if (!(std::fabs(x[i] - e) <= 1e-9 * (b - a))) return false;
    }
    return true;
}
int cs_table_upload(cs_ctx *ctx, int table_slot, int64_t nnu, const double *nu, int nT, const double *T, int nP, const double *P,
                    const double *lnsigma)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (table_slot < 0 || table_slot >= CS_MAX_TABLE) return fail(CS_EINVAL, "table slot %d out of range", table_slot);
    if (nT < 2 || nP < 2 || !T || !P || !lnsigma) return fail(CS_EINVAL, "need at least 2 x 2 grid points");
    int rc;
    if ((rc = check_ascending(nu, nnu))) return rc;
    for (int i = 1; i < nT; i++)
        if (!(T[i] > T[i - 1])) return fail(CS_EORDER, "table temperatures must be ascending");
    for (int j = 0; j < nP; j++)
        if (!(P[j] > 0) || (j > 0 && !(P[j] > P[j - 1]))) return fail(CS_EORDER, "table pressures must be positive and ascending");
    // the interpolant's barycentric weights (cheb_basis) are those of Chebyshev extrema: on any other grid the result would not be the
    // interpolating polynomial.  Omega.T and Omega.P are chebygrid(Tmin, Tmax, nT) and exp.(chebygrid(ln Pmin, ln Pmax, nP)), gases.jl:57-58
    {
        std::vector<double> lnP(nP);
        for (int j = 0; j < nP; j++) lnP[j] = std::log(P[j]);
        if (!cheb_extrema(T, nT)) return fail(CS_EINVAL, "table temperatures are not the Chebyshev extrema of [%g, %g] (Omega.T, gases.jl:57)", T[0], T[nT - 1]);
        if (!cheb_extrema(lnP.data(), nP)) return fail(CS_EINVAL, "table pressures are not the Chebyshev extrema in ln P of [%g, %g] (Omega.P, gases.jl:58)", P[0], P[nP - 1]);
    }
    const size_t n = (size_t)nT * nP * nnu;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(lnsigma[i])) return fail(CS_EINVAL, "ln sigma must be finite (OpacityTable stores ln(floatmin) for empty rows, gases.jl:76-80)");
    HIPCHK(hipSetDevice(ctx->device));
    TableDev &tb = ctx->tab[table_slot];
    tb.present = false;
    if ((rc = upload(tb.Z, lnsigma, n, ctx->stream))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    tb.nnu = nnu; tb.nT = nT; tb.nP = nP;
    tb.T.assign(T, T + nT);
    tb.lnP.resize(nP);
    for (int j = 0; j < nP; j++) tb.lnP[j] = std::log(P[j]);
    tb.nu.assign(nu, nu + nnu);
    tb.generation = next_generation();
    tb.present = true;
    return CS_OK;
}

int cs_accel_upload(cs_ctx *ctx, int accel_slot, int64_t nnu, const double *nu, int nk, const double *P_knots, const double *lnsigma)
{
    if (!ctx) return fail(CS_EINVAL, "ctx is NULL");
    if (accel_slot < 0 || accel_slot >= CS_MAX_ACCEL) return fail(CS_EINVAL, "accelerated-absorber slot %d out of range", accel_slot);
    if (nk < 2 || !P_knots || !lnsigma) return fail(CS_EINVAL, "need at least two pressure knots");
    int rc;
    if ((rc = check_ascending(nu, nnu))) return rc;
    for (int k = 0; k < nk; k++)
        if (!(P_knots[k] > 0) || (k > 0 && !(P_knots[k] > P_knots[k - 1]))) return fail(CS_EORDER, "knot pressures must be positive and strictly ascending");
    HIPCHK(hipSetDevice(ctx->device));
    AccelDev &ad = ctx->accel[accel_slot];
    const bool resident_here = ctx->col.ready && ctx->col.accel.slot == accel_slot;
    if (resident_here && (ad.nk != nk || ad.nnu != nnu)) ctx->col.ready = false;   // (its knot cells belong to the old knots)
    std::vector<double> lnP(nk);
    for (int k = 0; k < nk; k++) lnP[k] = std::log(P_knots[k]);
    // other knots (or another grid) than the slot held: a resident column's knot cells are stale (column_current refuses them until
    // cs_column_set_accel forms new ones); the same knots with new values -- what update! leaves -- keep the generation
    const bool same_knots = ad.present && ad.nk == nk && ad.nnu == nnu && ad.lnP == lnP && std::equal(ad.nu.begin(), ad.nu.end(), nu);
    ad.present = false;
    if ((rc = upload(ad.L, lnsigma, (size_t)nk * nnu, ctx->stream))) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!same_knots) ad.generation = next_generation();
    ad.nnu = nnu;
    ad.nk = nk;
    ad.nu.assign(nu, nu + nnu);
    ad.lnP = lnP;
    ad.present = true;
    return CS_OK;
}

int cs_accel_fetch(cs_ctx *ctx, int accel_slot, int64_t nnu, int nk, double *lnsigma)
{
    if (!ctx || accel_slot < 0 || accel_slot >= CS_MAX_ACCEL || !ctx->accel[accel_slot].present) return fail(CS_EINVAL, "accelerated-absorber slot is empty");
    const AccelDev &ad = ctx->accel[accel_slot];
    if (!lnsigma || nnu != ad.nnu || nk != ad.nk)
        return fail(CS_ESTATE, "the slot holds %lld wavenumbers x %d knots, caller expects %lld x %d", (long long)ad.nnu, ad.nk, (long long)nnu, nk);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(lnsigma, ad.L.p, (size_t)nk * nnu * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return CS_OK;
}

namespace {
struct MappedFile {
    const char *p = nullptr;
    size_t len = 0;
    int fd = -1;
    ~MappedFile()
    {
        if (p) munmap((void *)p, len);
        if (fd >= 0) close(fd);
    }
    int open_ro(const char *fn)
    {
        fd = ::open(fn, O_RDONLY);
        if (fd < 0) return fail(CS_EINVAL, "cannot open %s", fn);
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size == 0) return fail(CS_EINVAL, "cannot stat %s (or empty file)", fn);
        len = (size_t)st.st_size;
        void *m = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) return fail(CS_EINVAL, "cannot map %s", fn);
        p = (const char *)m;
        return CS_OK;
    }
};

// a mapped .par file and the offsets of its records (cs_par.h: the layout half of the validity rule); refusals say what first, the file
// name after it, where a long path cannot push the record and field out of the message
struct ParFile {
    MappedFile f;
    std::vector<size_t> off;
    int open(const char *fn)
    {
        int rc = f.open_ro(fn);
        if (rc) return rc;
        std::string err;
        if (!cs_par::index_records(f.p, f.len, off, err)) return fail(CS_EINVAL, "%s (%s)", err.c_str(), fn);
        return CS_OK;
    }
    int64_t n() const { return (int64_t)off.size(); }
    int parse(const char *fn, const cs_par::Arrays &o) const   // (the field half)
    {
        std::string err;
        if (!cs_par::parse_records(f.p, off, o, err)) return fail(CS_EINVAL, "%s (%s)", err.c_str(), fn);
        return CS_OK;
    }
};
}  // namespace

int cs_par_count(const char *filename, int64_t *n)
{
    if (!filename || !n) return fail(CS_EINVAL, "bad arguments");
    ParFile pf;
    int rc = pf.open(filename);
    if (rc) return rc;
    *n = pf.n();
    return CS_OK;
}

int cs_par_parse(const char *filename, int64_t n, int16_t *M, char *I, double *nu, double *S, double *A, double *gamma_a,
                 double *gamma_s, double *Epp, double *na, double *delta_a)
{
    if (!filename) return fail(CS_EINVAL, "bad arguments");
    ParFile pf;
    int rc = pf.open(filename);
    if (rc) return rc;
    if (pf.n() != n) return fail(CS_EINVAL, "file holds %lld records, caller expects %lld", (long long)pf.n(), (long long)n);
    return pf.parse(filename, {M, I, {nu, S, A, gamma_a, gamma_s, Epp, na, delta_a}});
}

using cs_par::iso_index;

int cs_gas_upload_par(cs_ctx *ctx, int slot, const char *filename, double numin, double numax, double Scut, const int *iso_keep,
                      int n_iso_keep, int64_t maxlines, int M_expected, const double *mu_table, int niso, const int32_t *ncheb,
                      const double *cheb, int64_t *L_out)
{
    if (!ctx || !filename || !mu_table || !ncheb || !cheb || niso < 1) return fail(CS_EINVAL, "bad arguments");
    int rc;
    ParFile pf;   // a file that breaks the rule is refused here, before the slot is touched: the table it holds stays as it was
    if ((rc = pf.open(filename))) return rc;
    const int64_t n = pf.n();
    std::vector<int16_t> M(n);
    std::vector<char> I(n);
    std::vector<double> nu(n), S(n), A(n), ga(n), gs(n), Epp(n), na(n), da(n);
    if ((rc = pf.parse(filename, {M.data(), I.data(), {nu.data(), S.data(), A.data(), ga.data(), gs.data(), Epp.data(), na.data(), da.data()}})))
        return rc;
    // par.jl:153-175: wavenumber range, intensity cut, isotopologue list
    std::vector<int64_t> keep;
    keep.reserve(n);
    for (int64_t i = 0; i < n; i++) {
        if (!(nu[i] >= numin && nu[i] <= numax && S[i] >= Scut)) continue;
        if (n_iso_keep > 0) {
            const int ii = iso_index(I[i]);
            bool ok = false;
            for (int q = 0; q < n_iso_keep; q++) ok = ok || iso_keep[q] == ii;
            if (!ok) continue;
        }
        keep.push_back(i);
    }
    if (keep.empty()) return fail(CS_EINVAL, "par information has been filtered to nothing!");   // par.jl:172
    // par.jl:177-186: the `maxlines` strongest lines (N is the unfiltered count there); order of equal intensities as the host
    // mirror produces it: ascending stable sort, reversed
    if (maxlines > 0 && n > maxlines) {
        std::stable_sort(keep.begin(), keep.end(), [&](int64_t a, int64_t b) { return S[a] < S[b]; });
        std::reverse(keep.begin(), keep.end());
        if ((int64_t)keep.size() > maxlines) keep.resize((size_t)maxlines);
    }
    std::stable_sort(keep.begin(), keep.end(), [&](int64_t a, int64_t b) { return nu[a] < nu[b]; });   // par.jl:188-191
    const int64_t L = (int64_t)keep.size();
    std::vector<double> o_nu(L), o_S(L), o_ga(L), o_gs(L), o_E(L), o_na(L), o_mu(L), o_da(L);
    std::vector<int16_t> o_iso(L);
    for (int64_t j = 0; j < L; j++) {
        const int64_t i = keep[j];
        if (M[i] != M_expected)   // SpectralLines holds one molecule (par.jl:239); the MOLPARAM rows handed in belong to M_expected
            return fail(CS_EINVAL, "record %lld is molecule %d, expected %d: SpectralLines objects must contain only one molecule's lines",
                        (long long)i, (int)M[i], M_expected);
        const int ii = iso_index(I[i]);
        if (ii < 1 || ii > niso) return fail(CS_EINVAL, "isotopologue '%c' of record %lld has no MOLPARAM row (%d rows)", I[i], (long long)i, niso);
        o_nu[j] = nu[i]; o_S[j] = S[i]; o_ga[j] = ga[i]; o_gs[j] = gs[i]; o_E[j] = Epp[i]; o_na[j] = na[i]; o_da[j] = da[i];
        o_iso[j] = (int16_t)ii;
        o_mu[j] = mu_table[ii - 1];
    }
    if (L_out) *L_out = L;
    if ((rc = cs_gas_upload(ctx, slot, L, o_nu.data(), o_S.data(), o_ga.data(), o_gs.data(), o_E.data(), o_na.data(), o_mu.data(), o_iso.data(),
                            niso, ncheb, cheb)))
        return rc;
    return attach_shift(ctx, slot, L, o_da.data());   // the file's own air pressure shifts (CS_SHAPE_PSHIFT)
}

int cs_gas_fetch(cs_ctx *ctx, int slot, int64_t L, double *nu, double *S, double *gamma_a, double *gamma_s, double *Epp, double *na,
                 double *mu_iso, int16_t *iso)
{
    if (!ctx || slot < 0 || slot >= CS_MAX_GAS || !ctx->gas[slot].present) return fail(CS_EINVAL, "gas slot is empty");
    GasTable &G = ctx->gas[slot];
    if (L != G.L) return fail(CS_EINVAL, "slot holds %lld lines, caller expects %lld", (long long)G.L, (long long)L);
    HIPCHK(hipSetDevice(ctx->device));
    const size_t nb = (size_t)L * sizeof(double);
    if (nu) HIPCHK(hipMemcpy(nu, G.nu.p, nb, hipMemcpyDeviceToHost));
    if (S) HIPCHK(hipMemcpy(S, G.S.p, nb, hipMemcpyDeviceToHost));
    if (gamma_a) HIPCHK(hipMemcpy(gamma_a, G.ga.p, nb, hipMemcpyDeviceToHost));
    if (gamma_s) HIPCHK(hipMemcpy(gamma_s, G.gs.p, nb, hipMemcpyDeviceToHost));
    if (Epp) HIPCHK(hipMemcpy(Epp, G.Epp.p, nb, hipMemcpyDeviceToHost));
    if (na) HIPCHK(hipMemcpy(na, G.na.p, nb, hipMemcpyDeviceToHost));
    if (mu_iso) HIPCHK(hipMemcpy(mu_iso, G.mu.p, nb, hipMemcpyDeviceToHost));
    if (iso) HIPCHK(hipMemcpy(iso, G.iso.p, (size_t)L * sizeof(int16_t), hipMemcpyDeviceToHost));
    return CS_OK;
}

// ---- multi-GPU --------------------------------------------------------------------------------------------
namespace {
// Host threads that drive the contexts of cs_fluxes_discretized_multi, kept for the life of the process: a thread's first HIP call
// costs milliseconds (per-thread runtime state), which a thread spawned per call would pay on every radiate!.
class WorkerPool {
    struct Worker {
        std::mutex m;
        std::condition_variable cv;
        std::function<void()> job;
        bool ready = false, done = true, quit = false;
        std::thread th;
    };
    std::vector<std::unique_ptr<Worker>> w_;
    std::mutex run_m_;
    static void loop(Worker *w)
    {
        for (;;) {
            std::unique_lock<std::mutex> lk(w->m);
            w->cv.wait(lk, [&] { return w->ready || w->quit; });
            if (w->quit) return;
            w->ready = false;
            std::function<void()> job = std::move(w->job);
            lk.unlock();
            job();
            lk.lock();
            w->done = true;
            w->cv.notify_all();
        }
    }
public:
    // f(0) on the calling thread, f(1) .. f(n-1) on workers; returns when all are through
    void run(int n, const std::function<void(int)> &f)
    {
        std::lock_guard<std::mutex> g(run_m_);
        while ((int)w_.size() < n - 1) {   // (parked on their condition variables between calls; joined by stop())
            w_.emplace_back(new Worker());
            w_.back()->th = std::thread(loop, w_.back().get());
        }
        for (int i = 1; i < n; i++) {
            Worker *w = w_[i - 1].get();
            std::lock_guard<std::mutex> lk(w->m);
            w->job = [&f, i] { f(i); };
            w->done = false;
            w->ready = true;
            w->cv.notify_all();
        }
        f(0);
        for (int i = 1; i < n; i++) {
            Worker *w = w_[i - 1].get();
            std::unique_lock<std::mutex> lk(w->m);
            w->cv.wait(lk, [&] { return w->done; });
        }
    }
    // end and join every worker (cs_destroy of the process's last context: a long-lived host session does not keep parked threads
    // that have touched the GPU; the next multi-context call starts new ones)
    void stop()
    {
        std::lock_guard<std::mutex> g(run_m_);
        for (auto &w : w_) {
            { std::lock_guard<std::mutex> lk(w->m); w->quit = true; w->cv.notify_all(); }
            if (w->th.joinable()) w->th.join();
        }
        w_.clear();
    }
};
WorkerPool &worker_pool()
{
    static WorkerPool *p = new WorkerPool();   // (never destroyed itself: no static-destruction order to get wrong)
    return *p;
}
}  // namespace
static void pool_stop() { worker_pool().stop(); }

// cost per wavenumber, as a running sum: a fixed part (flux sweeps, interpolation carry, setup) + per gas its local line density rho
// [lines per cm^-1 within +-2 cm^-1] x (0.011 + 1.1e-6 nu) -- near-line pairs grow with the Doppler width.  The constants were fitted
// to the kernel times of the eight 1/8 shards of BASELINE configs[2] (profiles/r02_notes.md, r03_notes.md); a column whose balance
// they miss is re-cut from measured times (cs_rebalance_ranges).
static void model_cost_sum(int64_t nnu, const double *nu, int ngas, const int64_t *nlines, const double *const *line_nu, std::vector<double> &cum)
{
    cum.assign((size_t)nnu + 1, 0.0);
    std::vector<int64_t> lo(ngas, 0), hi(ngas, 0);   // nu ascends (asserted by the callers of the product path; any order still works,
    for (int64_t i = 0; i < nnu; i++) {              // the two cursors just move both ways): lines in [nu - 2, nu + 2] by two cursors per gas
        double w = 0.19;
        for (int gq = 0; gq < ngas; gq++) {
            const double *t = line_nu[gq];
            const int64_t L = nlines[gq];
            int64_t &a = lo[gq], &b = hi[gq];
            while (a < L && t[a] < nu[i] - 2.0) a++;
            while (a > 0 && t[a - 1] >= nu[i] - 2.0) a--;
            while (b < L && t[b] <= nu[i] + 2.0) b++;
            while (b > 0 && t[b - 1] > nu[i] + 2.0) b--;
            w += (double)(b - a) / 4.0 * (0.011 + 1.1e-6 * nu[i]);
        }
        cum[i + 1] = cum[i] + w;
    }
}
// nparts contiguous non-empty ranges of equal cost from the running cost sum; edges on multiples of 64 points where the grid allows
static int cut_equal_cost(int64_t nnu, const std::vector<double> &cum, int nparts, int64_t *ranges)
{
    std::vector<int64_t> edge(nparts + 1);
    const bool tiles = nnu >= (int64_t)64 * 4 * nparts;   // range edges on multiples of 64 points (the kernels' tile) where the grid allows
    for (int r = 0; r <= nparts; r++) {
        int64_t e = std::lower_bound(cum.begin(), cum.end(), cum[nnu] * r / nparts) - cum.begin();
        if (tiles) e = (e + 32) / 64 * 64;
        edge[r] = e;
    }
    edge[0] = 0;
    edge[nparts] = nnu;
    // every part keeps at least one point (one tile where edges sit on tiles): push edges up from the left, then down from the right
    const int64_t step = tiles ? 64 : 1;
    for (int r = 1; r < nparts; r++) edge[r] = std::max(edge[r], edge[r - 1] + step);
    for (int r = nparts - 1; r >= 1; r--) edge[r] = std::min(edge[r], edge[r + 1] - (r == nparts - 1 ? 1 : step));
    for (int r = 1; r < nparts; r++) edge[r] = std::max(edge[r], edge[r - 1] + 1);
    for (int r = 0; r < nparts; r++) {
        if (!(edge[r] >= 0 && edge[r] < edge[r + 1] && edge[r + 1] <= nnu)) return fail(CS_EINVAL, "could not cut %lld wavenumbers into %d non-empty ranges", (long long)nnu, nparts);
        ranges[2 * r] = edge[r];
        ranges[2 * r + 1] = edge[r + 1];
    }
    return CS_OK;
}

int cs_balanced_ranges(int64_t nnu, const double *nu, int ngas, const int64_t *nlines, const double *const *line_nu, int nparts, int64_t *ranges)
{
    if (!nu || nnu < 1 || nparts < 1 || !ranges || ngas < 0 || (ngas > 0 && (!nlines || !line_nu))) return fail(CS_EINVAL, "bad arguments");
    if (nparts > nnu) return fail(CS_EINVAL, "more parts (%d) than wavenumbers (%lld)", nparts, (long long)nnu);
    std::vector<double> cum;
    model_cost_sum(nnu, nu, ngas, nlines, line_nu, cum);
    return cut_equal_cost(nnu, cum, nparts, ranges);
}

int cs_rebalance_ranges(int64_t nnu, const double *nu, int ngas, const int64_t *nlines, const double *const *line_nu, int nparts,
                        const int64_t *prev_ranges, const double *prev_time, double fixed_time, int64_t *ranges)
{
    if (!nu || nnu < 1 || nparts < 1 || !ranges || !prev_ranges || !prev_time || ngas < 0 || (ngas > 0 && (!nlines || !line_nu)))
        return fail(CS_EINVAL, "bad arguments");
    if (nparts > nnu) return fail(CS_EINVAL, "more parts (%d) than wavenumbers (%lld)", nparts, (long long)nnu);
    for (int r = 0; r < nparts; r++) {
        const bool ok = prev_ranges[2 * r] == (r ? prev_ranges[2 * r - 1] : 0) && prev_ranges[2 * r + 1] > prev_ranges[2 * r] &&
                        prev_time[r] > 0.0 && std::isfinite(prev_time[r]);
        if (!ok || (r == nparts - 1 && prev_ranges[2 * r + 1] != nnu))
            return fail(CS_EINVAL, "prev_ranges must be a partition of the grid into %d non-empty ranges with positive measured times", nparts);
    }
    if (!(fixed_time >= 0.0)) return fail(CS_EINVAL, "fixed_time must be >= 0");
    std::vector<double> cum, cal((size_t)nnu + 1, 0.0);
    model_cost_sum(nnu, nu, ngas, nlines, line_nu, cum);
    // the model's density, rescaled part by part so that it reproduces what the part took beyond the share that does not move with the
    // edges; a part the model under-rates gets denser and will shrink
    for (int r = 0; r < nparts; r++) {
        const int64_t a = prev_ranges[2 * r], b = prev_ranges[2 * r + 1];
        const double t = std::max(prev_time[r] - fixed_time, 0.05 * prev_time[r]);
        const double sc = t / std::max(cum[b] - cum[a], 1e-300);
        for (int64_t i = a; i < b; i++) cal[i + 1] = cal[i] + (cum[i + 1] - cum[i]) * sc;
    }
    return cut_equal_cost(nnu, cal, nparts, ranges);
}

int cs_fluxes_discretized_multi(cs_ctx *const *ctxs, int nctx, int64_t nnu, const double *nu, int np, const double *P, double g, int nlobatto,
                                const double *T_nodes, const double *mu_nodes, const double *T_levels, int ngas, const int *gas_slots,
                                const int *shapes, const double *dnu_cuts, const double *conc, double sigma_gray, const double *sigma_extra,
                                const double *S_toa, const double *albedo, double theta_s, int nstream, double *tau, double *Mup,
                                double *Mdn, double *Fup, double *Fdn)
{
    if (!ctxs || nctx < 1) return fail(CS_EINVAL, "no contexts");
    for (int i = 0; i < nctx; i++)
        if (!ctxs[i]) return fail(CS_EINVAL, "context %d is NULL", i);
    if (!nu || !P || nnu < 1 || np < 2 || !Fup || !Fdn) return fail(CS_EINVAL, "bad grid arguments");
    if (nctx == 1)
        return cs_fluxes_discretized(ctxs[0], nnu, nu, np, P, g, nlobatto, T_nodes, mu_nodes, T_levels, ngas, gas_slots, shapes, dnu_cuts, conc,
                                     sigma_gray, sigma_extra, S_toa, albedo, theta_s, nstream, tau, Mup, Mdn, Fup, Fdn);
    int rc;
    if ((rc = check_ascending(nu, nnu))) return rc;
    if (nlobatto < 2 || nlobatto > CS_MAX_LOBATTO) return fail(CS_EINVAL, "nlobatto must be in [2,%d]", CS_MAX_LOBATTO);
    // the partition: equal estimated device time per context, from the line tables the first context holds (every context must hold
    // the same tables in the same slots)
    std::vector<int64_t> nl_(ngas), ranges(2 * (size_t)nctx);
    std::vector<const double *> ln_(ngas);
    for (int gi = 0; gi < ngas; gi++) {
        const int sl = gas_slots[gi];
        if (sl < 0 || sl >= CS_MAX_GAS) return fail(CS_EINVAL, "gas slot %d out of range", sl);
        for (int i = 0; i < nctx; i++)
            if (!ctxs[i]->gas[sl].present || ctxs[i]->gas[sl].L != ctxs[0]->gas[sl].L)
                return fail(CS_EINVAL, "gas slot %d must hold the same table on every context (context %d differs)", sl, i);
        nl_[gi] = ctxs[0]->gas[sl].L;
        ln_[gi] = ctxs[0]->gas[sl].h_nu.data();
    }
    // (partition and weights of an unchanged grid and gas line-up are kept by the first context: radiate! calls this once per time step)
    MultiPlan &mp = ctxs[0]->mplan;
    std::vector<uint64_t> gens(ngas);
    for (int gi = 0; gi < ngas; gi++) gens[gi] = ctxs[0]->gas[gas_slots[gi]].generation;
    bool calibrate = false;
    if (!(mp.nctx == nctx && (int64_t)mp.nu.size() == nnu && mp.gens == gens && memcmp(mp.nu.data(), nu, (size_t)nnu * sizeof(double)) == 0)) {
        if ((rc = cs_balanced_ranges(nnu, nu, ngas, nl_.data(), ln_.data(), nctx, ranges.data()))) return rc;
        // a new plan: once, inside this call, the model's partition is re-cut from what its ranges are measured to take on THIS column
        // (cs_rebalance_ranges) -- where every context has a device to itself, so that a range's time is its own (Settings::multi_recut
        // of the first context: also on shared devices, for tests)
        calibrate = ngas > 0;
        for (int i = 0; i < nctx && calibrate; i++)
            for (int q = 0; q < i; q++)
                if (ctxs[q]->device == ctxs[i]->device) calibrate = false;
        if (ctxs[0]->set.multi_recut) calibrate = ngas > 0;
        mp.nctx = nctx;
        mp.nu.assign(nu, nu + nnu);
        mp.gens = gens;
        mp.ranges = ranges;
        mp.wt.resize(nnu);   // trapezoid weights of the WHOLE grid (util.jl:26-33): shards use slices, so their band fluxes simply add
        for (int64_t j = 0; j < nnu; j++) mp.wt[j] = ((j > 0 ? nu[j] - nu[j - 1] : 0.0) + (j + 1 < nnu ? nu[j + 1] - nu[j] : 0.0)) / 2;
    }
  for (int pass = 0; pass < 2; pass++) {
    ranges = mp.ranges;
    const std::vector<double> &wt = mp.wt;
    std::vector<double> run_ms(nctx, 0.0);
    const int K = (np - 1) * (nlobatto - 1) + 1, nl = np - 1;
    std::vector<int> rcs(nctx, CS_OK);
    std::vector<std::string> msgs(nctx);
    // Contexts that share a device (several ranges per card) take turns at the kernels, in context order: range i + 1 starts when the
    // kernels of range i are through, so that the copy-back of one range -- tau, M+, M- are 24 bytes per spectral point over PCIe --
    // runs beside the kernels of the next instead of all ranges finishing, then copying, together.  Different devices run side by side.
    std::vector<int> prev(nctx, -1);
    for (int i = 0; i < nctx; i++)
        for (int q = 0; q < i; q++)
            if (ctxs[q]->device == ctxs[i]->device) prev[i] = q;
    std::mutex turn_m;
    std::condition_variable turn_cv;
    std::vector<char> kernels_done(nctx, 0);
    std::vector<double> Fpart((size_t)nctx * 2 * np, 0.0);
    // one host thread per context (persistent workers): its uploads, kernels and copy-backs run beside the others' (a context is not
    // re-entrant, but different contexts are independent; HIP calls carry their device through hipSetDevice per thread)
    auto work = [&](int i) {
        cs_ctx *ctx = ctxs[i];
        const int64_t a = ranges[2 * i], n = ranges[2 * i + 1] - a;
        std::vector<double> ex;
        if (sigma_extra) {   // [nnu, K] nu-fastest -> this shard's columns
            ex.resize((size_t)n * K);
            for (int k = 0; k < K; k++) std::copy(sigma_extra + (size_t)k * nnu + a, sigma_extra + (size_t)k * nnu + a + n, ex.begin() + (size_t)k * n);
        }
        const double gl = a > 0 ? nu[a - 1] : 0.0, gr = a + n < nnu ? nu[a + n] : 0.0;
        int r;
        if (column_matches(ctx, n, nu + a, np, P, g, nlobatto, ngas, gas_slots, shapes, dnu_cuts, sigma_gray, theta_s, nstream, tau ? CS_TAU_LAYERS : CS_TAU_NONE,
                           (Mup || Mdn) ? CS_M_PLANES : CS_M_NONE, nnu, a, gl, gr)) {
            Column &c = ctx->col;
            hipStream_t s = ctx->stream;
            r = hipSetDevice(ctx->device) == hipSuccess ? CS_OK : fail(CS_EHIP, "hipSetDevice(%d) failed", ctx->device);
            drop_graph(c);   // (spectra may have been switched on or off: other kernel arguments)
            c.has_extra = sigma_extra != nullptr;
            c.has_S = S_toa != nullptr && std::any_of(S_toa + a, S_toa + a + n, [](double x) { return x != 0.0; });
            c.has_alb = albedo != nullptr && std::any_of(albedo + a, albedo + a + n, [](double x) { return x != 0.0; });
            if (!r && c.has_extra) r = upload(c.extra, ex.data(), ex.size(), s);
            if (!r && c.has_S) r = upload(c.S_toa, S_toa + a, n, s);
            if (!r && c.has_alb) r = upload(c.albedo, albedo + a, n, s);
            if (!r) r = cs_column_update_state(ctx, T_nodes, mu_nodes, T_levels, conc, nullptr);
        } else {
            r = cs_column_setup(ctx, n, nu + a, wt.data() + a, np, P, g, nlobatto, T_nodes, mu_nodes, T_levels, ngas, gas_slots, shapes, dnu_cuts,
                                conc, sigma_gray, sigma_extra ? ex.data() : nullptr, S_toa ? S_toa + a : nullptr, albedo ? albedo + a : nullptr,
                                theta_s, nstream, tau ? CS_TAU_LAYERS : CS_TAU_NONE, (Mup || Mdn) ? CS_M_PLANES : CS_M_NONE);
            if (!r) { ctx->col.g_nnu = nnu; ctx->col.g_start = a; ctx->col.g_left = gl; ctx->col.g_right = gr; }
        }
        if (prev[i] >= 0) {
            std::unique_lock<std::mutex> lk(turn_m);
            turn_cv.wait(lk, [&] { return kernels_done[prev[i]] != 0; });
        }
        if (!r) r = cs_column_run(ctx, nullptr);
        if (!r && hipStreamSynchronize(ctx->stream) != hipSuccess) r = fail(CS_EHIP, "hipStreamSynchronize failed");
        if (!r && calibrate && pass == 0) {   // the range's own time: a second, warm evaluation (the first one loaded code objects)
            const auto t0 = std::chrono::steady_clock::now();
            r = cs_column_run(ctx, nullptr);
            if (!r && hipStreamSynchronize(ctx->stream) != hipSuccess) r = fail(CS_EHIP, "hipStreamSynchronize failed");
            run_ms[i] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        {
            std::lock_guard<std::mutex> lk(turn_m);
            kernels_done[i] = 1;   // (also on failure: nobody is left waiting)
        }
        turn_cv.notify_all();
        if (!r) r = cs_column_fetch(ctx, n, np, tau ? tau + (size_t)a * nl : nullptr, Mup ? Mup + (size_t)a * np : nullptr,
                                    Mdn ? Mdn + (size_t)a * np : nullptr, Fpart.data() + (size_t)i * 2 * np, Fpart.data() + (size_t)i * 2 * np + np);
        rcs[i] = r;
        if (r) msgs[i] = g_err;   // (thread-local: carry it to the caller's thread)
    };
    worker_pool().run(nctx, work);
    for (int i = 0; i < nctx; i++)
        if (rcs[i]) return fail(rcs[i], "context %d (device %d): %s", i, ctxs[i]->device, msgs[i].c_str());
    if (calibrate && pass == 0) {
        calibrate = false;
        std::vector<int64_t> re(2 * (size_t)nctx);
        const double fixed = 0.3 * *std::min_element(run_ms.begin(), run_ms.end());   // (the launch chain of a step: does not move with the edges)
        if (cs_rebalance_ranges(nnu, nu, ngas, nl_.data(), ln_.data(), nctx, mp.ranges.data(), run_ms.data(), fixed, re.data()) == CS_OK && re != mp.ranges) {
            mp.ranges = re;
            continue;   // the call's results come from the re-cut partition, like every later call's
        }
    }
    for (int l = 0; l < np; l++) {   // fixed-order host sum: bitwise repeatable (SURVEY 8e's deterministic alternative to an all-reduce)
        double u = 0.0, d = 0.0;
        for (int i = 0; i < nctx; i++) { u += Fpart[(size_t)i * 2 * np + l]; d += Fpart[(size_t)i * 2 * np + np + l]; }
        Fup[l] = u;
        Fdn[l] = d;
    }
    return CS_OK;
  }
    return CS_OK;
}

int cs_streamnodes(int n, double *m, double *W)
{
    if (n < 1 || n > CS_MAX_STREAM) return fail(CS_EINVAL, "nstream must be in [1,%d]", CS_MAX_STREAM);
    double x[CS_MAX_STREAM], w[CS_MAX_STREAM];
    gauss_legendre(n, x, w);
    for (int i = 0; i < n; i++) {  // core/shared.jl:10-19
        const double th = (M_PI / 2) * (x[i] + 1) / 2;
        const double wi = (M_PI / 2) * w[i] / 2;
        m[i] = 1 / std::cos(th);
        W[i] = 2 * M_PI * wi * std::cos(th) * std::sin(th);
    }
    return CS_OK;
}

int cs_lobattonodes(int n, double *xs, double *ws)
{
    if (n < 2 || n > CS_MAX_LOBATTO) return fail(CS_EINVAL, "nlobatto must be in [2,%d]", CS_MAX_LOBATTO);
    double x[CS_MAX_LOBATTO], w[CS_MAX_LOBATTO];
    gauss_lobatto(n, x, w);
    for (int i = 0; i < n; i++) {  // core/discretized.jl:6-7
        xs[i] = (x[i] + 1) / 2;
        ws[i] = w[i] / 2;
    }
    return CS_OK;
}

int cs_devfn_batch(cs_ctx *ctx, int which, int64_t n, const double *x, const double *y, const double *z, double *out)
{
    if (!ctx || n < 0 || which < 0 || which > 2 || !x || !out) return fail(CS_EINVAL, "bad arguments");
    if ((which >= 1 && !y) || (which == 2 && !z)) return fail(CS_EINVAL, "this function takes more arguments");
    if (n == 0) return CS_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf dx, dy, dz, dout;
    int rc;
    if ((rc = upload(dx, x, n, s)) || (y && (rc = upload(dy, y, n, s))) || (z && (rc = upload(dz, z, n, s)))) return rc;
    HIPCHK(dout.reserve(n * sizeof(double)));
    CS_LAUNCH(k_devfn, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, which, n, dx.as<double>(), dy.as<double>(), dz.as<double>(), dout.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CS_OK;
}

int cs_faddeeva_batch(cs_ctx *ctx, int64_t n, const double *x, const double *y, double *out)
{
    if (!ctx || n < 0) return fail(CS_EINVAL, "bad arguments");
    if (n == 0) return CS_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = upload(ctx->tmpA, x, n, s)) || (rc = upload(ctx->tmpB, y, n, s))) return rc;
    HIPCHK(ctx->tmpC.reserve(n * sizeof(double)));
    CS_LAUNCH(k_faddeeva, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, ctx->tmpA.as<double>(),
                       ctx->tmpB.as<double>(), ctx->tmpC.as<double>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, ctx->tmpC.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return CS_OK;
}

}  // extern "C"
