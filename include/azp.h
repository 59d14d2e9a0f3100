/*
 * azp.h -- C ABI of libazp: MI355X (gfx950) force-compute kernels for the
 * azplugins pair / bond potentials.
 *
 * This is the drop-in boundary. Every entry point replaces one kernel-driver
 * template instantiation that the reference (stattlab/azplugins v1.1.0)
 * requests from HOOMD-blue v5:
 *
 *   azp_pair_forces_*            <- hoomd::md::kernel::gpu_compute_pair_forces<E>
 *                                   (src/PotentialPairGPUKernel.cu.inc:25-28)
 *   azp_dpd_forces_general_weight<- gpu_compute_dpd_forces<DPDPairEvaluatorGeneralWeight>
 *                                   (src/PotentialPairDPDThermoGPUKernel.cu.inc:21-24)
 *   azp_aniso_forces_two_patch_morse
 *                                <- gpu_compute_pair_aniso_forces<AnisoPairEvaluatorTwoPatchMorse>
 *                                   (src/AnisoPotentialPairGPUKernel.cu.inc:21-25)
 *   azp_bond_forces_*            <- gpu_compute_bond_forces<E, 2>
 *                                   (src/PotentialBondGPUKernel.cu.inc:25-29)
 *   azp_angle_forces_*           (no counterpart in the reference: HOOMD's md.angle conventions, defined here)
 *   azp_dihedral_forces_*        (no counterpart in the reference: md.dihedral's names, semantics defined here)
 *   azp_pair_forces_table, azp_bond_forces_table
 *                                (no counterpart in the reference: md.pair.Table / md.bond.Table, semantics defined here)
 *   azp_angle_forces_table, azp_dihedral_forces_table, azp_bonded_histogram
 *                                (no counterpart in the reference: md.angle.Table / md.dihedral.Table and the
 *                                   distributions they are inverted from, semantics defined here)
 *
 * Conventions (all restated from HOOMD-blue's ForceCompute data model):
 *   - Scalar = double. Scalar4 arrays are 4 consecutive doubles.
 *   - d_pos[i]   = (x, y, z, type) with the integer type index stored in the
 *                  low 32 bits of w (HOOMD __scalar_as_int).
 *   - d_force[i] = (fx, fy, fz, energy); energy is this particle's half share.
 *   - d_virial   = 6 rows (xx, xy, xz, yy, yz, zz) of length virial_pitch.
 *   - d_orientation[i] = quaternion, scalar part first.
 *   - neighbor list: full storage; neighbors of i are
 *     d_nlist[d_head_list[i] + k], k < d_n_neigh[i]; indices may point at
 *     ghost particles (>= N, < n_max).
 *   - per-type-pair tables (rcutsq, ronsq, params) are indexed
 *     type_i * ntypes + type_j and must be symmetric.
 *   - outputs are OVERWRITTEN for all N local particles.
 *   - all pointers prefixed d_ are device pointers borrowed for the call. The
 *     bond, DPD, aniso, barrier, wall, NVE, neighbor-list and generic pair kernels
 *     allocate nothing and never synchronise the stream; azp_pair_plan_build,
 *     azp_pair_plan_build_from_cells and the plan cache behind azp_pair_forces_*
 *     (see there) own device workspace and synchronise.
 *   - every function returns 0 on success, a positive hipError_t value if the
 *     launch failed, or a negative azp_status for invalid arguments; nothing
 *     throws across this boundary.
 */
#ifndef AZP_H_
#define AZP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZP_VERSION_MAJOR 0
#define AZP_VERSION_MINOR 2

typedef enum azp_status
    {
    AZP_SUCCESS = 0,
    AZP_ERROR_INVALID_ARGUMENT = -1,
    AZP_ERROR_TOO_MANY_TYPES = -2, /* per-type-pair table does not fit in LDS; a pair call returns it only when the
                                      generic kernel's table does not fit either (a tile kernel that cannot hold the
                                      table beside its staged slots hands the call to the generic kernel) */
    AZP_ERROR_NO_DEVICE = -3,
    AZP_ERROR_TOO_MANY_BINS = -4   /* velocity field: more than 2^31 - 1 bins */
    } azp_status;

typedef enum azp_shift_mode
    {
    AZP_SHIFT_NONE = 0,
    AZP_SHIFT_SHIFT = 1,
    AZP_SHIFT_XPLOR = 2
    } azp_shift_mode;

/* HOOMD BoxDim fields the kernels need: box centred on the origin. */
typedef struct azp_box
    {
    double L[3];
    double tilt[3]; /* xy, xz, yz */
    int32_t periodic[3];
    int32_t _pad;
    } azp_box;

/* ---- parameter structs: byte-compatible with the reference's param_type ---- */

/* src/PairEvaluatorPerturbedLennardJones.h:57-66 */
typedef struct azp_plj_params { double sigma_6, epsilon_x_4, attraction_scale_factor, rwcasq; } azp_plj_params;
/* src/PairEvaluatorHertz.h:41-47 */
typedef struct azp_hertz_params { double epsilon; } azp_hertz_params;
/* src/PairEvaluatorExpandedYukawa.h:44-53 (aligned(32)) */
typedef struct azp_yukawa_params { double epsilon, kappa, delta, _pad; } azp_yukawa_params;
/* src/PairEvaluatorColloid.h:48-57 */
typedef struct azp_colloid_params { double A, a_1, a_2, sigma_3; } azp_colloid_params;
/* src/DPDPairEvaluatorGeneralWeight.h:53-62 (aligned(32)) */
typedef struct azp_dpd_params { double A, gamma, s, _pad; } azp_dpd_params;
/* src/AnisoPairEvaluatorTwoPatchMorse.h:63-69 */
typedef struct azp_tpm_params { double M_d, M_rinv, r_eq, omega, alpha; uint8_t repulsion; uint8_t _pad[7]; } azp_tpm_params;
/* src/BondEvaluatorDoubleWell.h:52-61 */
typedef struct azp_dw_params { double r_1, r_diff, U_1, U_tilt; } azp_dw_params;
/* src/BondEvaluatorQuartic.h:68-82 */
typedef struct azp_quartic_params { double k, r_0, b_1, b_2, U_0, sigma_6, epsilon_x_4, delta; } azp_quartic_params;

/* Tabulated potentials (no counterpart in the reference: HOOMD's md.pair.Table / md.bond.Table names, semantics
 * DEFINED HERE). A table has n intervals of equal length dr from r_min: knots r_k = r_min + k dr,
 * k = 0..n, with values U_k and F_k = -dU/dr at r_k (F is supplied by the user, not derived). For
 * r_min <= r < r_min + n dr:
 *     s = (r - r_min) / dr,  k = min(floor(s), n - 1),  f = s - k,
 *     U(r) = U_k + f (U_{k+1} - U_k),  F(r) = F_k + f (F_{k+1} - F_k),  force_divr = F(r) / r.
 * d_rows: n rows of four doubles {U_k, U_{k+1} - U_k, F_k, F_{k+1} - F_k} in device memory, 32-byte aligned
 * (azp_table_pack writes them): one 32-byte read per evaluation, no read of row k + 1.
 *   pair (azp_pair_forces_table): n = width, dr = (r_cut - r_min) / width with r_cut from d_rcutsq (r_max is ignored);
 *     the value at r_cut is not stored, U_n = F_n = 0 is folded into row n - 1. r < r_min or r >= r_cut: nothing.
 *     r_cut = 0, n = 0 or d_rows = NULL: the type pair is never evaluated.
 *   bond (azp_bond_forces_table): n = width - 1, dr = (r_max - r_min) / n, both end points stored. r < r_min or
 *     r >= r_max (or n = 0, d_rows = NULL, r_max <= r_min): the evaluator rejects the bond BEFORE any table read and
 *     the kernel raises *d_flags ("bond out of bounds"). */
typedef struct azp_table_params
    {
    double r_min;
    double r_max;         /* bonds; ignored for pairs */
    const double* d_rows; /* n x 4, device memory */
    uint32_t n;           /* intervals */
    uint32_t _pad;
    } azp_table_params;
/* Host function: `width` samples U, F -> rows. closed = 0 (pair form): the samples are the knots 0 .. width - 1 of
 * width intervals on [r_min, r_end), the knot at r_end is the implicit zero; width rows are written. closed = 1 (bond
 * form): the samples are all knots of width - 1 intervals on [r_min, r_end]; width - 1 rows are written.
 * AZP_ERROR_INVALID_ARGUMENT (nothing written): a NULL pointer, width < 1 (closed: < 2), r_min < 0 or not finite,
 * r_end <= r_min or not finite, a non-finite U or F. */
int azp_table_pack(double r_min, double r_end, const double* U, const double* F, uint32_t width, int closed, double* out_rows);

/* Host-side construction / inspection of the parameter structs: what the
 * reference does in each struct's pybind11::dict constructor and asDict() /
 * toPython() (file:line next to each struct above). Pure host functions. */
void azp_plj_params_make(double epsilon, double sigma, double attraction_scale_factor, azp_plj_params* out);
void azp_plj_params_unpack(const azp_plj_params* p, double* epsilon, double* sigma, double* attraction_scale_factor);
void azp_colloid_params_make(double A, double a_1, double a_2, double sigma, azp_colloid_params* out);
void azp_colloid_params_unpack(const azp_colloid_params* p, double* A, double* a_1, double* a_2, double* sigma);
void azp_tpm_params_make(double M_d, double M_r, double r_eq, double omega, double alpha, int repulsion,
                         azp_tpm_params* out);
void azp_tpm_params_unpack(const azp_tpm_params* p, double* M_d, double* M_r, double* r_eq, double* omega,
                           double* alpha, int* repulsion);
void azp_dw_params_make(double r_0, double r_1, double U_1, double U_tilt, azp_dw_params* out);
void azp_dw_params_unpack(const azp_dw_params* p, double* r_0, double* r_1, double* U_1, double* U_tilt);
void azp_quartic_params_make(double k, double r_0, double b_1, double b_2, double U_0, double sigma, double epsilon,
                             double delta, azp_quartic_params* out);
void azp_quartic_params_unpack(const azp_quartic_params* p, double* k, double* r_0, double* b_1, double* b_2,
                               double* U_0, double* sigma, double* epsilon, double* delta);

/* ---- pair forces ---- */

#define AZP_PAIR_FLAG_NO_AUTO_PLAN 1u /* azp_pair_forces_*: always the generic kernel (no cached tile plan) */

/* Mirrors hoomd::md::kernel::pair_args_t (minus charge and devprop). */
typedef struct azp_pair_args
    {
    double* d_force;             /* N x 4, overwritten                              */
    double* d_virial;            /* 6 x virial_pitch, overwritten if compute_virial */
    uint64_t virial_pitch;
    uint32_t N;                  /* local particles                                 */
    uint32_t n_max;              /* local + ghost particles addressable in d_pos    */
    const double* d_pos;         /* n_max x 4                                       */
    azp_box box;
    const uint32_t* d_n_neigh;   /* N                                               */
    const uint32_t* d_nlist;
    const uint64_t* d_head_list; /* N                                               */
    const double* d_rcutsq;      /* ntypes^2                                        */
    const double* d_ronsq;       /* ntypes^2 (xplor only; may be NULL otherwise)    */
    uint64_t size_nlist;         /* total entries in d_nlist (0 = unknown; tuning hint) */
    uint32_t ntypes;
    uint32_t shift_mode;         /* azp_shift_mode                                  */
    uint32_t compute_virial;
    uint32_t block_size;         /* 0 = library default                             */
    uint32_t threads_per_particle; /* 0 = library heuristic; else 1,2,4,8,16,32     */
    uint32_t flags;              /* AZP_PAIR_FLAG_*                                 */
    uint32_t range_first;        /* compute only particles [range_first, range_first + */
    uint32_t range_count;        /* range_count); range_count = 0 means all N. Lets a   */
                                 /* caller overlap the ghost exchange with the interior */
                                 /* particles (planned kernels round outwards to tiles) */
    double r_list_max;           /* optional: upper bound on the separation of any
                                    listed pair (r_cut_max + 2 r_buff); lets interior
                                    particles skip the minimum-image step. 0 = unknown. */
    const double* d_rinnersq;    /* optional, read by azp_pair_plan_build only: ntypes^2
                                    inner radii^2. Listed pairs closer than this when the
                                    plan is built are placed first in their rows, so that
                                    an evaluator's short-range branch (PerturbedLJ: the WCA
                                    core, r < 2^(1/6) sigma) is confined to the first chunks
                                    of a row. Ordering hint only; NULL = none.           */
    uint32_t has_displacement_bound; /* 0 (default): unknown, whole rows are processed        */
    uint32_t _pad3;
    double displacement_bound;   /* when has_displacement_bound != 0, read by the *_planned
                                    entry points: an upper bound on the distance ANY particle
                                    (local or ghost) has moved since azp_pair_plan_build. Rows
                                    end with the Verlet-buffer entries, split by their
                                    separation r_b at build time; an entry with
                                    r_b >= r_cut + m cannot be in range while
                                    2 * displacement_bound <= m, so the kernel stops before
                                    them (exact, not a heuristic):
                                      bound == 0 (positions unchanged): every buffer entry
                                            is skipped;
                                      2 * bound <= r_buff / 2: the outer half of the buffer
                                            shell is skipped (needs r_list_max at plan build);
                                      larger: whole rows.
                                    HOOMD: max |x - x_at_last_nlist_update|, the quantity
                                    NeighborList::distanceCheck compares with r_buff / 2.    */
    const float* d_displacement; /* optional (with has_displacement_bound != 0), read by the *_planned entry
                                    points: n_max per-particle upper bounds on the distance each particle has moved
                                    since the positions the plan's row classes refer to (azp_nlist_displacements
                                    writes them next to the global maximum). A tile of the kernel then stops its rows
                                    at the shells ITS OWN members and listed neighbors can have crossed (twice the
                                    largest of their displacements) instead of what the fastest particle of the whole
                                    system dictates. Exact; NULL = the global bound alone.  */
    uint64_t list_generation;    /* optional, read by the entry points that keep their own plan cache (azp_pair_forces_*,
                                    azp_dpd_forces_general_weight, azp_aniso_forces_two_patch_morse): a number the caller
                                    changes whenever it rewrites the neighbor list (HOOMD: NeighborList::getNumUpdates()
                                    + 1). Non-zero: the cached plan is recompiled exactly when the number changes and the
                                    list is not fingerprinted; 0 = unknown, the list is fingerprinted at every call. */
    const uint32_t* d_stale_flag; /* optional, read by the *_planned entry points together with the next field: the two
                                    words azp_nlist_distance_check / azp_nlist_displacements leave in device memory
                                    (d_flag and d_max_dist_sq_bits). The kernel then takes its displacement bound from
                                    there AT RUN TIME (sqrt of the double whose bits are in *d_displacement_sq_bits, plus
                                    displacement_bound_extra), and its workgroups leave at once when *d_stale_flag != 0
                                    (some particle moved farther than the check's limit: the list has to be rebuilt and
                                    the call repeated). A caller can so queue the force kernel right behind the check,
                                    before the host knows its result. has_displacement_bound / displacement_bound are
                                    ignored when these are set. */
    const unsigned long long* d_displacement_sq_bits;
    double displacement_bound_extra; /* added to every d_displacement entry: how far any particle had moved from those
                                    reference positions when the plan was built (0 in the usual flow: plan and list are
                                    built from the same positions) */
    } azp_pair_args;

/* The five entry points below take what gpu_compute_pair_forces<E> takes and nothing
 * else. With threads_per_particle == 0 (library's choice) they run the LDS-staged tile
 * kernel from a plan that libazp compiles and caches by itself (csrc/pair_auto.hpp): each
 * call fingerprints the list on the device (row lengths, row starts, cutoffs, box; the
 * entries themselves for lists of up to 2^22 entries, sampled beyond), measures the
 * largest displacement since the plan was compiled, reads the result (<= 24 KiB) back (ONE stream
 * synchronisation per call) and recompiles the plan when the list changed. A caller that
 * passes an explicit threads_per_particle (HOOMD's autotuner value), or sets
 * AZP_PAIR_FLAG_NO_AUTO_PLAN, or runs with AZP_AUTO_PLAN=0 in the environment, gets the
 * generic kernel, which never synchronises. Callers that know when the list changes use
 * the azp_pair_plan_* API below instead and pay neither check nor readback. */
int azp_pair_forces_perturbed_lennard_jones(const azp_pair_args* args, const azp_plj_params* d_params, void* stream);
int azp_pair_forces_hertz(const azp_pair_args* args, const azp_hertz_params* d_params, void* stream);
int azp_pair_forces_expanded_yukawa(const azp_pair_args* args, const azp_yukawa_params* d_params, void* stream);
int azp_pair_forces_colloid(const azp_pair_args* args, const azp_colloid_params* d_params, void* stream);
/* PotentialPairConservativeGeneralWeight (src/export_PotentialPairDPDThermo.cc.inc:33-35) */
int azp_pair_forces_dpd_conservative(const azp_pair_args* args, const azp_dpd_params* d_params, void* stream);
/* Tabulated pair potential (azp_table_params above). shift_mode must be AZP_SHIFT_NONE: AZP_ERROR_INVALID_ARGUMENT
 * otherwise. The rows every d_params entry points at are borrowed for the call like d_params itself. */
int azp_pair_forces_table(const azp_pair_args* args, const azp_table_params* d_params, void* stream);

/* ---- tile plan: compiled neighbor list for the LDS-staged pair kernel ----
 * The generic azp_pair_forces_* kernels gather every neighbor position through
 * L1/L2. When the particle order is spatially sorted (HOOMD's SFC sorter), a
 * plan lets the kernels stage each tile's neighbor positions once in LDS and
 * address them with 16-bit tile-local indices (see csrc/pair_plan.hpp).
 * Build the plan whenever the neighbor list was rebuilt (HOOMD:
 * NeighborList::getNumUpdates() changed) -- it synchronises the stream and may
 * (re)allocate device workspace owned by the plan -- then call the *_planned
 * entry points every step. If the list cannot be tiled (a tile's neighbor set
 * exceeds 2559 particles or a row exceeds ~1000 entries, e.g. unsorted particle order) the plan is marked
 * invalid and the planned entry points run the generic kernel instead. Tiles
 * that are wide compared with the box, triclinic boxes, or calls without the
 * r_list_max hint re-apply the minimum image per pair (slower, still exact).
 * Results agree with the generic kernel to rounding. */
typedef struct azp_pair_plan azp_pair_plan; /* opaque */

typedef struct azp_pair_plan_info
    {
    int32_t valid;
    int32_t invalid_reason;      /* 0 none, 2: a tile lists more than 2559 distinct neighbors (or a row is too long);
                                    3, 4, 5: see azp_pair_plan_build_from_cells */
    uint32_t threads_per_particle;
    uint32_t tile_size;          /* particles per tile (workgroup) */
    uint32_t lds_slots;          /* staged-position capacity the kernel is instantiated for */
    uint32_t n_tiles;
    uint32_t max_stage;          /* largest staged set over all tiles */
    uint32_t max_row;            /* azp_pair_plan_build_from_cells: longest row found */
    uint64_t total_stage;        /* sum of staged-set sizes */
    uint64_t compiled_bytes;     /* size of the compiled 16-bit list */
    uint64_t builds;
    int32_t from_cells;          /* 1: compiled by azp_pair_plan_build_from_cells */
    uint32_t row_capacity;       /* ... with rows of this many entries */
    uint64_t list_id, head_id;   /* ... pass these as azp_pair_args.d_nlist / d_head_list to the *_planned
                                    entry points (the plan is its own list; there is no u32 list) */
    int32_t balanced;            /* 1: rows handed to the lanes in the order of their in-range lengths
                                    (azp_pair_plan_set_balance) */
    float core_radius;           /* ordering class and diagnostic (one particle type; no kernel consumes it): entries outside
                                    row class "core" were at least this far apart when the plan was built; 0: no such class */
    float sure_radius;           /* ... entries of row class "sure" at most this far apart; 0: no such class */
    uint32_t max_member_cells;   /* azp_pair_plan_build_from_cells, cells of the full list radius: the largest number of
                                    distinct cells the members of one tile sit in (beyond 128 the plan is refused with
                                    reason 4). It grows as the particles diffuse away from their sorted order: a caller
                                    that re-sorts them when it approaches the limit never sees the refusal */
    } azp_pair_plan_info;

int azp_pair_plan_create(azp_pair_plan** out);
void azp_pair_plan_destroy(azp_pair_plan* plan);
int azp_pair_plan_build(azp_pair_plan* plan, const azp_pair_args* args, void* stream);
/* Build option of azp_pair_plan_build_from_cells (default off): within every tile of 256 particles the
 * rows are handed to the force kernel's lanes longest in-range row first, so that each of its four waves
 * gets rows of similar in-range length. The tile kernels run as many heavy per-pair blocks per wave as
 * the LONGEST in-range row of the wave has entries; for potentials whose pair block is expensive and
 * whose rows are short and ragged (DPD thermostat: Philox per pair, 12.6 +- 3 in range) that is the
 * difference between max-over-256 and the quartile maxima. Results are those of the unbalanced plan. */
int azp_pair_plan_set_balance(azp_pair_plan* plan, int enabled);
/* Diagnostics: the staged-set size of the first n tiles of the last build (host copy, no device access);
 * returns the number of entries written. */
int azp_pair_plan_tile_stage(const azp_pair_plan* plan, uint32_t* out, uint32_t n);
/* (azp_pair_plan_build_from_cells, the plan compiled straight from the cell list, is declared with the
 * neighbor-list entry points below.) */
/* Build option: order every row bank-aware (conflict-poor LDS gathers; default on).
 * It adds ~10 % to the build and buys ~2-3 % per force call, so it pays for lists that
 * live for more than ~50 force calls; callers that rebuild more often turn it off. */
int azp_pair_plan_set_bank_order(azp_pair_plan* plan, int enabled);
int azp_pair_plan_query(const azp_pair_plan* plan, azp_pair_plan_info* info);
/* Diagnostics (copies from the device, synchronises; no kernel consumes the phase counts): the row classes of the
 * last build as means over the slices -- out[0] chunks that cover the core entries, out[1] chunks up to the end of
 * the all-sure part of the rows, out[2] chunks of the whole rows. */
int azp_pair_plan_phase_chunks(const azp_pair_plan* plan, float out[3]);
/* Row ends of a plan. The Verlet-buffer entries of every row are ordered into azp_pair_plan_shells() shells of equal
 * width by their separation at build time; per slice (one wave of the force kernel: 4 per tile) the plan keeps
 * shells + 1 counts of BATCHES -- 4 entries per lane, half a 16-byte chunk -- that cover the in-range entries [0] and
 * the entries up to the end of shell s [1 + s]; the last one is the whole row. A launch that has to walk n shells
 * (azp_pair_plan_shells_for: the smallest n with n x width >= 2 x bound, all of them without a bound, with a NaN or
 * negative one, or without a width) runs count / 2 whole iterations and, for an odd count, one half iteration.
 * azp_pair_plan_row_batches copies the first n counts of the last build from the device (synchronises), stores the
 * shell width (optional) and returns the number of counts written (0: no valid plan). Diagnostics and tests. */
uint32_t azp_pair_plan_shells(void);
uint32_t azp_pair_plan_shells_for(double shell_width, int has_bound, double bound);
int azp_pair_plan_row_batches(const azp_pair_plan* plan, uint32_t* out, uint32_t n, double* shell_width);

/* The plan cache behind azp_pair_forces_* (diagnostics and tests). */
typedef struct azp_auto_plan_stats
    {
    uint64_t calls;             /* calls that went through the cache                  */
    uint64_t compiles;          /* plan compilations (list changed / first use)      */
    uint64_t reuses;            /* calls served by an unchanged plan                 */
    uint64_t generic_fallbacks; /* calls whose list could not be tiled               */
    } azp_auto_plan_stats;
void azp_pair_auto_plan_get_stats(azp_auto_plan_stats* out);
void azp_pair_auto_plan_clear(void); /* frees every cached plan (synchronises the device) */

int azp_pair_forces_planned_perturbed_lennard_jones(azp_pair_plan* plan, const azp_pair_args* args,
                                                    const azp_plj_params* d_params, void* stream);
int azp_pair_forces_planned_hertz(azp_pair_plan* plan, const azp_pair_args* args, const azp_hertz_params* d_params,
                                  void* stream);
int azp_pair_forces_planned_expanded_yukawa(azp_pair_plan* plan, const azp_pair_args* args,
                                            const azp_yukawa_params* d_params, void* stream);
int azp_pair_forces_planned_colloid(azp_pair_plan* plan, const azp_pair_args* args, const azp_colloid_params* d_params,
                                    void* stream);
int azp_pair_forces_planned_dpd_conservative(azp_pair_plan* plan, const azp_pair_args* args,
                                             const azp_dpd_params* d_params, void* stream);
int azp_pair_forces_planned_table(azp_pair_plan* plan, const azp_pair_args* args, const azp_table_params* d_params,
                                  void* stream);

/* Mirrors hoomd::md::kernel::dpd_pair_args_t. */
typedef struct azp_dpd_args
    {
    azp_pair_args pair;
    const double* d_vel;   /* n_max x 4 (vx, vy, vz, mass) */
    const uint32_t* d_tag; /* n_max                        */
    uint64_t timestep;
    double deltaT;
    double T;              /* kT(timestep)                 */
    uint16_t seed;
    uint16_t _pad[3];
    } azp_dpd_args;

int azp_dpd_forces_general_weight(const azp_dpd_args* args, const azp_dpd_params* d_params, void* stream);
/* Tile-staged form: positions, velocities and tags of a tile's neighbors staged once in LDS
 * (csrc/xtiled.hpp); `plan` is compiled from args->pair with azp_pair_plan_build. Falls back to
 * the kernel above when the list cannot be tiled. */
int azp_dpd_forces_planned_general_weight(azp_pair_plan* plan, const azp_dpd_args* args, const azp_dpd_params* d_params,
                                          void* stream);

/* Mirrors hoomd::md::kernel::a_pair_args_t. */
typedef struct azp_aniso_args
    {
    azp_pair_args pair;
    const double* d_orientation; /* n_max x 4 */
    double* d_torque;            /* N x 4, overwritten */
    } azp_aniso_args;

int azp_aniso_forces_two_patch_morse(const azp_aniso_args* args, const azp_tpm_params* d_params, void* stream);
/* Tile-staged form: the patch director of every staged neighbor is computed once per tile
 * and kept in LDS with its position (csrc/xtiled.hpp). */
int azp_aniso_forces_planned_two_patch_morse(azp_pair_plan* plan, const azp_aniso_args* args, const azp_tpm_params* d_params,
                                             void* stream);

/* ---- bond forces ---- */

/* HOOMD group_storage<2>: one entry of the per-particle GPU bond table. */
typedef struct azp_bond_entry
    {
    uint32_t idx;  /* index of the other member of the bond */
    uint32_t type; /* bond type                             */
    } azp_bond_entry;

/* Mirrors hoomd::md::kernel::bond_args_t<2>. Table entry b of particle i is
 * d_gpu_bondlist[b * pitch + i], b < d_gpu_n_bonds[i]; d_gpu_bond_pos[b * pitch + i]
 * is i's position (0 or 1) inside that bond. */
typedef struct azp_bond_args
    {
    double* d_force;
    double* d_virial;
    uint64_t virial_pitch;
    uint32_t N;
    uint32_t n_max;
    const double* d_pos;
    azp_box box;
    const azp_bond_entry* d_gpu_bondlist;
    const uint32_t* d_gpu_bond_pos;
    const uint32_t* d_gpu_n_bonds;
    uint64_t pitch;
    uint32_t n_bond_types;
    uint32_t compute_virial;
    uint32_t block_size;
    uint32_t _pad;
    } azp_bond_args;

/* d_flags: one device word, set to 1 when an evaluator returned false
 * (invalid parameters) -- HOOMD turns that into "bond out of bounds". */
int azp_bond_forces_double_well(const azp_bond_args* args, const azp_dw_params* d_params, unsigned int* d_flags,
                                void* stream);
int azp_bond_forces_quartic(const azp_bond_args* args, const azp_quartic_params* d_params, unsigned int* d_flags,
                            void* stream);
/* Tabulated bond potential (azp_table_params above): a bond outside [r_min, r_max) raises *d_flags. */
int azp_bond_forces_table(const azp_bond_args* args, const azp_table_params* d_params, unsigned int* d_flags,
                          void* stream);

/* ---- special pair forces (azplugins_amd.special_pair) ----
 * Two-body potentials over a per-particle table of SPECIAL PAIRS: pairs of particles that carry an interaction of
 * their own, such as the scaled 1-4 pairs of an OPLS chain that the neighbor list excludes. The
 * reference holds no such code; the names are HOOMD's md.special_pair, the semantics are DEFINED HERE.
 *
 * The table has the layout of the bond table (azp_bond_entry: partner, type; the particle's position in the pair in
 * a plane of its own), and the kernel is the bond kernel with another evaluator: one lane per particle, no atomics,
 * each member gets F on itself, U / 2 and, when compute_virial is set, half of the pair's virial; two calls give the
 * same bits at every block size. With d the minimum-image separation and r = |d|:
 *   LJ   U = 4 epsilon [(sigma / r)^12 - (sigma / r)^6] for r^2 < r_cut^2, U = 0 and F = 0 otherwise. NO shift: U
 *        jumps at r_cut (HOOMD's md.special_pair.LJ). r = 0 is undefined.
 * azp_special_pair_lj_params holds lj1 = 4 epsilon sigma^12, lj2 = 4 epsilon sigma^6 and r_cut^2, folded on the host
 * in double; unpack returns sigma = (lj1 / lj2)^(1/6) and epsilon = lj2^2 / (4 lj1) (to rounding; 0, 0 where lj1 or
 * lj2 is 0). The evaluator cannot reject its parameters: there is no flag word. Error returns as for the angle kernel. */
typedef struct azp_special_pair_lj_params { double lj1, lj2, r_cutsq, _pad; } azp_special_pair_lj_params;

typedef struct azp_special_pair_args
    {
    double* d_force;         /* N x 4, overwritten */
    double* d_virial;        /* 6 x virial_pitch, written when compute_virial is set */
    uint64_t virial_pitch;
    uint32_t N;
    uint32_t n_max;
    const double* d_pos;     /* n_max x 4 */
    azp_box box;
    const azp_bond_entry* d_gpu_pairlist; /* entry s of particle i at s * pitch + i, s < d_gpu_n_pairs[i] */
    const uint32_t* d_gpu_pair_pos;       /* i's position (0 or 1) in that pair */
    const uint32_t* d_gpu_n_pairs;
    uint64_t pitch;
    uint32_t n_pair_types;
    uint32_t compute_virial;
    uint32_t block_size;     /* 0: 256; otherwise a multiple of 64, at most 256 */
    uint32_t _pad;
    } azp_special_pair_args;

void azp_special_pair_lj_params_make(double epsilon, double sigma, double r_cut, azp_special_pair_lj_params* out);
void azp_special_pair_lj_params_unpack(const azp_special_pair_lj_params* p, double* epsilon, double* sigma, double* r_cut);
int azp_special_pair_forces_lj(const azp_special_pair_args* args, const azp_special_pair_lj_params* d_params, void* stream);

/* ---- angle forces ----
 * Three-body bending potentials over a per-particle angle table. The reference holds no angle code; the semantics
 * are HOOMD's documented md.angle.Harmonic and md.angle.CosineSquared conventions, DEFINED HERE.
 *
 * An angle has members a, b, c with b the vertex. With dab = r_a - r_b and dcb = r_c - r_b (both minimum image):
 *   c = dab.dcb / (|dab| |dcb|), clamped to [-1, 1];   s = max(sqrt(1 - c^2), 1e-3)   (the floor is HOOMD's)
 * An evaluator yields U and g = dU/d(cos theta):
 *   harmonic         U = 1/2 k (theta - t0)^2, theta = acos(c);   g = -k (theta - t0) / s
 *   cosine squared   U = 1/2 k (c - cos t0)^2;                    g = k (c - cos t0)
 * Forces:  F_a = -g (dcb / (|dab||dcb|) - c dab / |dab|^2),  F_c = -g (dab / (|dab||dcb|) - c dcb / |dcb|^2),
 *          F_b = -F_a - F_c.
 * Each member gets U / 3 and, when compute_virial is set, the virial 1/3 (dab (x) F_a + dcb (x) F_c), stored in the
 * six rows xx, xy, xz, yy, yz, zz with the sign of the bond kernel. Coincident members (|dab| or |dcb| equal to 0)
 * are undefined. No atomics: one lane per particle sums its entries in table order, so two calls give the same bits.
 * A particle without angles gets exact zeros. */

/* One entry of the per-particle angle table (16 bytes, read as one load). */
typedef struct azp_angle_entry
    {
    uint32_t idx[2]; /* indices of the two other members, in angle order (a, b, c without this particle) */
    uint32_t type;   /* angle type                                                                       */
    uint32_t pos;    /* this particle's position in the angle: 0 = a, 1 = b (vertex), 2 = c              */
    } azp_angle_entry;

typedef struct azp_angle_harmonic_params { double k, t0; } azp_angle_harmonic_params;
/* cos t0 is folded on the host */
typedef struct azp_angle_cossq_params { double k, cos_t0; } azp_angle_cossq_params;

/* Table entry s of particle i is d_gpu_anglelist[s * pitch + i], s < d_gpu_n_angles[i]; only rows [0, N) have
 * entries, their partners are rows of [0, n_max). */
typedef struct azp_angle_args
    {
    double* d_force;         /* N x 4, overwritten */
    double* d_virial;        /* 6 x virial_pitch, written when compute_virial is set */
    uint64_t virial_pitch;
    uint32_t N;
    uint32_t n_max;
    const double* d_pos;     /* n_max x 4 */
    azp_box box;
    const azp_angle_entry* d_gpu_anglelist;
    const uint32_t* d_gpu_n_angles;
    uint64_t pitch;
    uint32_t n_angle_types;
    uint32_t compute_virial;
    uint32_t block_size;     /* 0: 256; otherwise a multiple of 64, at most 256 */
    uint32_t _pad;
    } azp_angle_args;

void azp_angle_harmonic_params_make(double k, double t0, azp_angle_harmonic_params* out);
void azp_angle_harmonic_params_unpack(const azp_angle_harmonic_params* p, double* k, double* t0);
void azp_angle_cossq_params_make(double k, double t0, azp_angle_cossq_params* out);
/* t0 comes back as acos(cos t0): equal to what was given to rounding, not to the bit */
void azp_angle_cossq_params_unpack(const azp_angle_cossq_params* p, double* k, double* t0);
/* No flag word: neither evaluator can reject its parameters. NULL args: AZP_ERROR_INVALID_ARGUMENT; N == 0: success,
 * nothing launched; a missing array, pitch < N, n_angle_types == 0, a block size that is no multiple of 64 or above
 * 256: AZP_ERROR_INVALID_ARGUMENT; parameters beyond 64 KiB of LDS: AZP_ERROR_TOO_MANY_TYPES. */
int azp_angle_forces_harmonic(const azp_angle_args* args, const azp_angle_harmonic_params* d_params, void* stream);
int azp_angle_forces_cosine_squared(const azp_angle_args* args, const azp_angle_cossq_params* d_params, void* stream);

/* ---- dihedral forces ----
 * Four-body torsion potentials over a per-particle dihedral table. The reference holds no dihedral code; the class
 * names and parameter keys are HOOMD's md.dihedral.Periodic and md.dihedral.OPLS, the semantics are DEFINED HERE
 * (DESIGN 4.17).
 *
 * A dihedral has members a, b, c, d. With b1 = r_b - r_a, b2 = r_c - r_b, b3 = r_d - r_c (each minimum image),
 * n1 = b1 x b2 and n2 = b2 x b3:
 *   phi = atan2(|b2| (b1 . n2), n1 . n2) in (-pi, pi]      (IUPAC: cis, a eclipsing d, is 0; trans is pi)
 * An evaluator yields U and U' = dU/dphi:
 *   periodic   U = 1/2 k (1 + d cos(n phi - phi0)),  d = +1 or -1, n an integer >= 1
 *   OPLS       U = 1/2 [k1 (1 + cos phi) + k2 (1 - cos 2 phi) + k3 (1 + cos 3 phi) + k4 (1 - cos 4 phi)]
 * Forces: F_m = -U' g_m with the gradient of phi (Blondel-Karplus form, no 1 / sin phi: phi = 0 and pi need no floor)
 *   s = (b1 . b2) / |b2|^2,  t = (b3 . b2) / |b2|^2,
 *   g_a = -(|b2| / |n1|^2) n1,   g_d = +(|b2| / |n2|^2) n2,
 *   g_b = -(1 + s) g_a + t g_d,  g_c = -(1 + t) g_d + s g_a.
 * The kernel takes cos phi = (n1 . n2) / (|n1||n2|) and sin phi = |b2| (b1 . n2) / (|n1||n2|) from the geometry and
 * the multiples of phi from the angle-addition recurrence; cos phi0 and sin phi0 are folded on the host.
 * Each member gets U / 4 and, when compute_virial is set, a quarter of
 *   W = (-b1) (x) F_a + b2 (x) F_c + (b2 + b3) (x) F_d
 * (the separations from b, composed from the three minimum-image vectors and not re-imaged), stored in the six rows
 * xx, xy, xz, yy, yz, zz with the sign of the bond kernel; the trace of W is zero. a, b, c or b, c, d collinear
 * (|n1| or |n2| equal to 0) and coincident members are undefined. No atomics: one lane per particle sums its entries
 * in table order, so two calls give the same bits. A particle without dihedrals gets exact zeros. */

/* One entry of the per-particle dihedral table (16 bytes, read as one load). */
typedef struct azp_dihedral_entry
    {
    uint32_t idx[3];   /* indices of the three other members, in dihedral order (a, b, c, d without this particle) */
    uint32_t type_pos; /* dihedral type in the low 30 bits; this particle's position 0 = a .. 3 = d in the top two  */
    } azp_dihedral_entry;

/* cos phi0 and sin phi0 are folded on the host */
typedef struct azp_dihedral_periodic_params
    {
    double k, cos_phi0, sin_phi0;
    int32_t d;  /* +1 or -1 */
    uint32_t n; /* >= 1     */
    } azp_dihedral_periodic_params;
typedef struct azp_dihedral_opls_params { double k1, k2, k3, k4; } azp_dihedral_opls_params;

/* Table entry s of particle i is d_gpu_dihedrallist[s * pitch + i], s < d_gpu_n_dihedrals[i]; only rows [0, N) have
 * entries, their partners are rows of [0, n_max). */
typedef struct azp_dihedral_args
    {
    double* d_force;         /* N x 4, overwritten */
    double* d_virial;        /* 6 x virial_pitch, written when compute_virial is set */
    uint64_t virial_pitch;
    uint32_t N;
    uint32_t n_max;
    const double* d_pos;     /* n_max x 4 */
    azp_box box;
    const azp_dihedral_entry* d_gpu_dihedrallist;
    const uint32_t* d_gpu_n_dihedrals;
    uint64_t pitch;
    uint32_t n_dihedral_types;
    uint32_t compute_virial;
    uint32_t block_size;     /* 0: 256; otherwise 64, 128 or 256 */
    uint32_t _pad;
    } azp_dihedral_args;

void azp_dihedral_periodic_params_make(double k, int d, unsigned int n, double phi0, azp_dihedral_periodic_params* out);
/* k, d and n come back exactly; phi0 as atan2(sin phi0, cos phi0): equal to what was given to rounding (for phi0 in
 * (-pi, pi]), not to the bit */
void azp_dihedral_periodic_params_unpack(const azp_dihedral_periodic_params* p, double* k, int* d, unsigned int* n, double* phi0);
void azp_dihedral_opls_params_make(double k1, double k2, double k3, double k4, azp_dihedral_opls_params* out);
void azp_dihedral_opls_params_unpack(const azp_dihedral_opls_params* p, double* k1, double* k2, double* k3, double* k4);
/* No flag word: neither evaluator can reject its parameters. NULL args: AZP_ERROR_INVALID_ARGUMENT; N == 0: success,
 * nothing launched; a missing array, pitch < N, n_dihedral_types == 0, a block size other than 64, 128 or 256:
 * AZP_ERROR_INVALID_ARGUMENT; parameters beyond 64 KiB of LDS: AZP_ERROR_TOO_MANY_TYPES. */
int azp_dihedral_forces_periodic(const azp_dihedral_args* args, const azp_dihedral_periodic_params* d_params, void* stream);
int azp_dihedral_forces_opls(const azp_dihedral_args* args, const azp_dihedral_opls_params* d_params, void* stream);

/* ---- tabulated angle and dihedral potentials (angle.Table, dihedral.Table) ----
 * The names are HOOMD's md.angle.Table and md.dihedral.Table; the reference holds no such code, the semantics are
 * DEFINED HERE. Both take azp_table_params (above) per type, with rows from azp_table_pack(closed = 1):
 * `width` >= 2 samples of the energy U and of the TORQUE tau = -dU/d(angle), both end points stored, n = width - 1
 * intervals, linear interpolation between the knots exactly as for the bond form (s, k = min(floor(s), n - 1),
 * f = s - k, U = U_k + f (U_{k+1} - U_k), tau likewise). The widths are per type. The whole domain of the angle is
 * covered, so nothing can be out of bounds: there is no flag word.
 *
 *   angle     knots theta_k = k pi / n on [0, pi]; r_min = 0, r_max = pi. With c and s = max(sin theta, 1e-3) of the
 *             angle geometry above: theta = acos(c), s_index = theta * (n / pi), g = dU/dc = tau / s. theta == pi
 *             gives s_index == n (or its neighbor in the last bit): the clamp k <= n - 1 then yields the value of the
 *             last knot, U = U_n.
 *   dihedral  knots phi_k = -pi + 2 pi k / n on [-pi, pi]; the table is packed and read over x = phi + pi in
 *             [0, 2 pi] (azp_table_pack refuses r_min < 0), r_min = 0, r_max = 2 pi. With cos phi and sin phi of the
 *             dihedral geometry above: phi = atan2(sin phi, cos phi), s_index = (phi + pi) * (n / (2 pi)),
 *             U' = dU/dphi = -tau. Periodicity is NOT enforced: U_0 may differ from U_n. Planar trans reads the end
 *             its sin phi names: sin phi = +0 gives phi = +pi and the LAST knot (U_n, tau_n), sin phi = -0 gives
 *             phi = -pi and the FIRST knot (U_0, tau_0). A table that is meant to be periodic stores equal ends.
 *
 * A type with n == 0 or d_rows == NULL contributes nothing (no energy, no force). Everything else -- the geometry, the
 * shares of energy and virial, the error returns -- is that of the analytic angle and dihedral entries above. */
int azp_angle_forces_table(const azp_angle_args* args, const azp_table_params* d_params, void* stream);
int azp_dihedral_forces_table(const azp_dihedral_args* args, const azp_table_params* d_params, void* stream);

/* ---- neighbor-list build (the step before the path) ----
 * Cell list -> full Verlet list in the layout the force kernels consume.
 * The reference consumes hoomd.md.nlist.Cell(buffer=...) (src/pytest/test_pair.py:337);
 * these kernels produce the same data: d_n_neigh, d_head_list (exclusive scan
 * of d_n_neigh, done by the caller) and d_nlist, rows compact and ordered by
 * cell, which is also the gather-friendly order for the force kernels.
 * Sequence: cell_assign -> (caller: stable sort of d_cell_of -> d_order,
 * d_cell_sorted) -> cell_bounds -> count -> (caller: exclusive scan) -> fill. */
typedef struct azp_cell_grid
    {
    double lo[3];        /* lower corner of the grid (fractional cells: in units of f, -0.5) */
    double width[3];     /* cell width, >= largest r_list (>= half of it with azp_nlist_args.cell_subdivision = 2);
                          * fractional cells: in units of f, 1 / dim, the slab of cells then >= r_list thick */
    uint32_t dim[3];
    int32_t periodic[3]; /* 1: cell index wraps; 0: clamped (ghost slab) */
    } azp_cell_grid;

typedef struct azp_nlist_args
    {
    uint32_t N;                 /* rows are built for particles [0, N)        */
    uint32_t n_total;           /* particles binned (local + ghosts)          */
    const double* d_pos;        /* n_total x 4                                */
    azp_box box;
    azp_cell_grid grid;
    uint32_t ntypes;
    /* 0 / 1: cells at least as wide as the largest r_list (every entry point). 2: cells at least HALF as wide
     * (azp_nlist_cell_assign / cell_bounds / bin and azp_pair_plan_build_from_cells only: the plan compiler then
     * searches the 5 x 5 x 5 cells around a particle's own, cut down per particle to the cells its list sphere
     * reaches -- 0.39 x the candidate tests; azp_nlist_count / fill refuse such cells) */
    uint32_t cell_subdivision;
    const double* d_rlistsq;    /* ntypes^2, (r_cut + r_buff)^2; <= 0 disables the pair */
    uint32_t* d_cell_of;        /* n_total, written by cell_assign            */
    const uint32_t* d_cell_sorted; /* n_total, d_cell_of in ascending order   */
    const uint32_t* d_order;    /* n_total, particle indices in that order    */
    uint32_t* d_cell_start;     /* ncell + 1, written by cell_bounds          */
    const uint32_t* d_n_excl;   /* optional: N exclusion counts (NULL = none) */
    const uint32_t* d_excl;     /* entry e of particle i at e * excl_pitch + i */
    uint64_t excl_pitch;
    uint32_t* d_n_neigh;        /* N, written by count                        */
    const uint64_t* d_head_list; /* N, read by fill                           */
    uint32_t* d_nlist;          /* written by fill                            */
    /* single-pass mode of azp_nlist_fill (HOOMD's own protocol: rows of fixed
     * capacity, rebuilt with larger rows on overflow): when row_capacity > 0 the
     * fill also writes d_n_neigh[i] (the full count), stores at most row_capacity
     * entries per row and raises *d_max_neigh to the largest count seen
     * (atomic max; the caller zeroes it before the launch and must rebuild with
     * larger rows if it exceeds row_capacity). row_capacity = 0: rows are exact
     * (head_list from a scan of the count pass). */
    uint32_t row_capacity;
    /* 0: Cartesian cells, grid.lo / grid.width in length units (orthorhombic boxes only for count / fill).
     * 1: fractional cells, parallelepipeds along the lattice vectors of `box`: particles are binned by
     *    f_z = z / Lz, f_y = (y - yz z) / Ly, f_x = (x - xy y - (xz - xy yz) z) / Lx, each in [-0.5, 0.5) for a wrapped
     *    particle; grid.lo = -0.5 and grid.width = 1 / dim in those units. Any box, tilted or not. Other values:
     *    AZP_ERROR_INVALID_ARGUMENT. */
    uint32_t fractional_cells;
    uint32_t* d_max_neigh;
    } azp_nlist_args;

int azp_nlist_cell_assign(const azp_nlist_args* args, void* stream);
int azp_nlist_cell_bounds(const azp_nlist_args* args, void* stream);
/* The binning in one call: d_cell_of, d_order (the particles cell by cell, ascending index inside a cell: what a
 * stable sort by cell gives) and d_cell_start are written (d_cell_sorted is not used). A counting sort: histogram,
 * scan, scatter, and a per-cell sort that makes the result independent of the order of the atomics. Scratch:
 * d_cursor (ncell words), d_order_tmp (n_total words; also holds the per-workgroup totals of the scan when the
 * grid has more than 32,768 cells). Grids of many small cells (cell_subdivision = 2) get a multi-workgroup scan
 * and a thread-per-cell sort. */
int azp_nlist_bin(const azp_nlist_args* args, uint32_t* d_cursor, uint32_t* d_order_tmp, void* stream);
/* The search reaches +-1 cell around a particle's own.
 * fractional_cells = 0 (Cartesian cells): orthorhombic boxes only -- across a periodic y or z face of a tilted box
 * the image of a neighbor is shifted by xy Ly (xz Lz, yz Lz), which is no whole number of cells. A box with a non-zero
 * tilt is refused with AZP_ERROR_INVALID_ARGUMENT before anything is launched or written.
 * fractional_cells = 1: any box. The caller chooses dim[k] <= w_k / r_list with the perpendicular widths
 * w_x = Lx / sqrt(1 + xy^2 + (xy yz - xz)^2), w_y = Ly / sqrt(1 + yz^2), w_z = Lz, so that a slab of cells is at least
 * r_list thick and two particles within r_list differ by at most one cell along every axis; a periodic axis needs
 * w_k >= 2 r_list (the minimum image is then unique). With fewer than 4 cells on some periodic axis the minimum image
 * is taken per pair; otherwise once per staged particle, relative to the home cell's centre in fractional
 * coordinates. An untilted box gives the same rows as Cartesian cells of the same dims.
 * cell_subdivision > 1 is refused by both kinds. azp_pair_plan_build_from_cells takes Cartesian cells of an
 * orthorhombic box only (invalid_reason 6 otherwise): for a tilted box fill the u32 list here and hand it to the force
 * kernels / azp_pair_plan_build. */
int azp_nlist_count(const azp_nlist_args* args, void* stream);
int azp_nlist_fill(const azp_nlist_args* args, void* stream);

/* The plan compiled straight from the cell list, in the pass that finds the neighbors
 * (csrc/pair_plan_cells.hip): no HOOMD-format list is produced or read. `cells`: the binned
 * particles as for azp_nlist_fill (d_pos, box, grid, d_rlistsq, d_cell_of, d_order,
 * d_cell_start, exclusions; d_n_neigh receives the row lengths; row_capacity = entries a row may
 * hold, 0 = 160; d_head_list / d_nlist / d_cell_sorted unused). `pair`: d_rcutsq, d_rinnersq,
 * r_list_max (required: sizes the buffer shells and decides where pairs must be re-imaged),
 * ntypes. Invalid plans (azp_pair_plan_query): invalid_reason 3 = a row exceeded row_capacity
 * (retry with max_row; hard limit 504), 2 = a tile stages more than 2559 particles, 4 / 5 =
 * particles not spatially sorted (the members of a tile of 256 sit in more than 128 cells, or
 * the cells around them number more than 512 / hold more than 8192 particles), 6 = tilted box,
 * fractional cells or more than 255 types -- build the u32 list and azp_pair_plan_build instead. The rows hold
 * the exact list plus, rarely, pairs a few 1e-6 r_list beyond it (single-precision acceptance
 * test with a margin that covers its own rounding); the force kernels' FP64 cutoff test ignores them. Synchronises the
 * stream once; owns device workspace (2 x row_capacity x 2 B per particle + the stage lists).
 * The *_planned entry points take list_id / head_id of azp_pair_plan_query as d_nlist /
 * d_head_list. */
int azp_pair_plan_build_from_cells(azp_pair_plan* plan, const azp_nlist_args* cells, const azp_pair_args* pair, void* stream);

/* Rebuild criterion (HOOMD NeighborList::distanceCheck restated): sets *d_flag to 1
 * when any of the n particles moved farther than sqrt(max_dist_sq) from its position
 * at the last build (minimum image in `box`); the caller zeroes *d_flag beforehand.
 * d_max_dist_sq_bits (optional, may be NULL; zeroed by the caller): receives the bit
 * pattern of the largest squared displacement as a double (atomic max on the bits,
 * which order like the values for non-negative doubles) -- the displacement bound the
 * planned force kernels accept (azp_pair_args.displacement_bound). */
int azp_nlist_distance_check(uint32_t n, const double* d_pos, const double* d_pos_at_build, const azp_box* box,
                             double max_dist_sq, uint32_t* d_flag, unsigned long long* d_max_dist_sq_bits, void* stream);
/* The same check that also writes every particle's own displacement (single precision, rounded up) to
 * d_displacement[0 .. n): the per-particle bounds azp_pair_args.d_displacement takes. */
int azp_nlist_displacements(uint32_t n, const double* d_pos, const double* d_pos_at_build, const azp_box* box,
                            double max_dist_sq, uint32_t* d_flag, unsigned long long* d_max_dist_sq_bits,
                            float* d_displacement, void* stream);

/* Sort keys of the particle sorter (the role of HOOMD's SFC sorter, which the tile plan relies
 * on): key of particle i = index of its cell along a blocked curve over a dims[0] x dims[1] x
 * dims[2] grid (block^3 cells per block, blocks and the cells inside them in row-major order), or,
 * with block = 0, the index along the Hilbert curve of a 2^b x 2^b x 2^b grid stretched over the box
 * (2^b >= the largest of dims, <= 1024); positions wrapped into the orthorhombic frame of `box`. */
int azp_sorter_keys(uint32_t n, const double* d_pos, const azp_box* box, const uint32_t* dims, uint32_t block, int32_t* d_keys,
                    void* stream);

/* ---- halo pack: dst[k, :] = src[idx[k], :] for k < n, rows of
 * row_doubles doubles (4 for positions / velocities / orientations). The send buffer of
 * the per-step ghost exchange; replaces the pack half of HOOMD's CommunicatorGPU. */
int azp_halo_pack(uint32_t n, const double* d_src, const int64_t* d_idx, uint32_t row_doubles, double* d_dst, void* stream);

/* Several per-particle arrays in ONE send buffer (DPD: positions + velocities + tags; aniso:
 * positions + orientations), so that a step needs a single collective. Packed row k holds, field
 * after field and each starting on an 8-byte boundary, row d_idx[k] of every field's array;
 * packed_row_bytes = sum of the fields' row sizes rounded up to 8. unpack writes packed row k to
 * row k of each field's destination (the caller passes the address of its first ghost row). */
#define AZP_HALO_MAX_FIELDS 4
typedef struct azp_halo_field
    {
    void* d_data;       /* pack: the source array; unpack: the first destination row */
    uint32_t row_bytes; /* bytes per particle, multiple of 4                         */
    uint32_t _pad;
    } azp_halo_field;
int azp_halo_pack_fields(uint32_t n, uint32_t n_fields, const azp_halo_field* fields, const int64_t* d_idx, void* d_packed,
                         uint32_t packed_row_bytes, void* stream);
int azp_halo_unpack_fields(uint32_t n, uint32_t n_fields, const azp_halo_field* fields, const void* d_packed,
                           uint32_t packed_row_bytes, void* stream);

/* ---- one-body harmonic barriers ----
 * Replaces the reference's own kernel driver
 *   azplugins::gpu::compute_harmonic_barrier<Evaluator>(...)   (src/HarmonicBarrierGPU.cuh:49-140,
 *   instantiated at src/HarmonicBarrierGPUKernel.cu.inc) for PlanarBarrierEvaluator
 *   (src/PlanarBarrierEvaluator.h:36-48) and SphericalBarrierEvaluator
 *   (src/SphericalBarrierEvaluator.h:36-51).
 * d_params: one (k, offset) pair per particle type (HOOMD Scalar2). Positions are
 * wrapped into the box before evaluation (src/HarmonicBarrier.h:167-169). The
 * virial is not computed by the reference (set to zero there); d_virial may be NULL. */
typedef struct azp_barrier_args
    {
    double* d_force;      /* N x 4, overwritten */
    double* d_virial;     /* 6 x virial_pitch, zeroed if not NULL */
    uint64_t virial_pitch;
    uint32_t N;
    uint32_t ntypes;
    const double* d_pos;  /* N x 4 */
    azp_box box;
    const double* d_params; /* ntypes x 2: k, offset */
    double location;      /* H (planar: y position) or R (spherical: radius) at this timestep */
    uint32_t block_size;
    uint32_t _pad;
    } azp_barrier_args;

int azp_external_planar_harmonic_barrier(const azp_barrier_args* args, void* stream);
int azp_external_spherical_harmonic_barrier(const azp_barrier_args* args, void* stream);
/* host-side validity checks of the evaluators (PlanarBarrierEvaluator::valid,
 * SphericalBarrierEvaluator::valid): 1 valid, 0 invalid */
int azp_planar_barrier_valid(double H, const azp_box* box);
int azp_spherical_barrier_valid(double R, const azp_box* box);

/* ---- velocity-Verlet NVE step ----
 * HOOMD's hoomd.md.methods.ConstantVolume without thermostat (the dummy
 * integrator of every reference test, src/pytest/test_pair.py:325-327), restated:
 * step one: v += a dt/2, x += v dt, wrap into the box (image counters updated);
 * step two: v += a dt/2 with the new net force. a = F / m, m = vel.w. */
typedef struct azp_nve_args
    {
    double* d_pos;            /* N x 4 (type in w is preserved) */
    double* d_vel;            /* N x 4 (vx, vy, vz, mass) */
    const double* d_net_force; /* N x 4 */
    int32_t* d_image;         /* N x 3 periodic image counters, may be NULL */
    azp_box box;
    double dt;
    uint32_t N;
    uint32_t block_size;
    } azp_nve_args;

int azp_integrate_nve_step_one(const azp_nve_args* args, void* stream);
int azp_integrate_nve_step_two(const azp_nve_args* args, void* stream);
/* Step two of one time step and step one of the next in one kernel: for a loop in which nothing reads the
 * velocities between the two (HOOMD calls integrateStepTwo and the next integrateStepOne back to back unless an
 * updater or analyzer is due). Same arithmetic in the same order as the two calls, one pass over the arrays. */
int azp_integrate_nve_step_two_one(const azp_nve_args* args, void* stream);
/* Net force of up to 8 force arrays (N x 4 each; HOOMD: Integrator::computeNetForce) in one pass:
 * d_out[i] = d_arrays[0][i] + d_arrays[1][i] + ... (d_arrays: HOST array of n_arrays device pointers). */
int azp_sum_forces(uint32_t n_rows, uint32_t n_arrays, const double* const* d_arrays, double* d_out, void* stream);

/* Rotational degrees of freedom of the same step ("+ rotational for
 * aniso"; the reference's aniso test gives its particles a moment of inertia,
 * src/pytest/test_pair_aniso.py:113-140): HOOMD's integrate_rotational_dof path restated -- the
 * symplectic NO_SQUISH quaternion scheme. q = d_orientation (scalar first), p = d_angmom (angular
 * momentum quaternion; body angular momentum = 1/2 conj(q) p), per-particle principal moments
 * d_inertia (N x 3; an axis with zero moment is not integrated), d_net_torque (N x 4, space
 * frame). step one: p += dt q t_body, free rotations about axes 3, 2, 1, 2, 3, q renormalised;
 * step two: p += dt q t_body. HOOMD-blue's source is absent here: PARITY UNPINNED (pinned by
 * conservation properties, tests/test_gpu_external_nve.py). */
typedef struct azp_nve_rot_args
    {
    double* d_orientation;      /* N x 4 */
    double* d_angmom;           /* N x 4 */
    const double* d_inertia;    /* N x 3 */
    const double* d_net_torque; /* N x 4 */
    double dt;
    uint32_t N;
    uint32_t block_size;
    } azp_nve_rot_args;

int azp_integrate_nve_rot_step_one(const azp_nve_rot_args* args, void* stream);
int azp_integrate_nve_rot_step_two(const azp_nve_rot_args* args, void* stream);

/* ---- Langevin and Brownian dynamics in a flow field ----
 * The integration methods of the reference's flow module (TwoStepLangevinFlow, TwoStepBrownianFlow, with the
 * ConstantFlow / ParabolicFlow fields), restated for HOOMD-blue v5:
 *   Langevin (src/TwoStepLangevinFlow.h:100-252)
 *     step one: x += (v + a dt/2) dt, wrap (image counters updated); v += a dt/2
 *     step two: R_k = -c + 2 c u01_k with c = sqrt(6 gamma kT / dt) (0 if noiseless);
 *               a = (F_net + R - gamma (v - u(x))) / m; v += a dt/2; a is stored in d_accel
 *   Brownian (src/TwoStepBrownianFlow.h:105-180), one call per time step:
 *     x += (u(x) + (F_net + R) / gamma) dt, wrap; velocities untouched.
 * gamma = d_gamma[type]. The random numbers come from Philox4x32-10 with key {id << 24 | (t >> 32 & 0xff) << 16 |
 * seed, t & 0xffffffff} and counter {k, tag, 0, 0} for draw k = 0, 1, 2 (id 202 Langevin, 201 Brownian,
 * src/RNGIdentifiers.h), u01 = (u64 >> 11) 2^-53 + 2^-54 of u64 = c0 << 32 | c1: the construction the DPD
 * thermostat uses. t = `timestep` is the time step at the start of the step the half belongs to.
 * Only rows [0, N) whose type t satisfies t < ntypes and (d_type_mask NULL or d_type_mask[t] != 0) are touched;
 * the Langevin force enters the acceleration only (never the net force, energies or virials). */
typedef enum azp_flow_kind
    {
    AZP_FLOW_CONSTANT = 0, /* u(r) = (p[0], p[1], p[2]) */
    AZP_FLOW_PARABOLIC = 1 /* u(r) = (p[0] (1 - (y / p[1])^2), 0, 0): p[0] = Umax = 1.5 U, p[1] = L = separation / 2 */
    } azp_flow_kind;

typedef struct azp_flow
    {
    uint32_t kind; /* azp_flow_kind */
    uint32_t _pad;
    double p[3];
    } azp_flow;

typedef struct azp_flow_method_args
    {
    double* d_pos;             /* N x 4 (type in w is preserved) */
    double* d_vel;             /* N x 4 (vx, vy, vz, mass) */
    double* d_accel;           /* N x 4 (ax, ay, az, unused); Langevin only, may be NULL for Brownian */
    const double* d_net_force; /* N x 4 */
    int32_t* d_image;          /* N x 3 periodic image counters, may be NULL */
    const uint32_t* d_tag;     /* N */
    const double* d_gamma;     /* ntypes friction coefficients */
    const uint8_t* d_type_mask; /* ntypes bytes, may be NULL (every type) */
    azp_box box;
    double dt;
    double kT;                 /* kT at `timestep` */
    uint64_t timestep;
    uint32_t seed;             /* low 16 bits used */
    uint32_t noiseless;
    uint32_t N;
    uint32_t ntypes;
    azp_flow flow;
    uint32_t block_size;       /* 0: 256 */
    uint32_t _pad;
    } azp_flow_method_args;

int azp_integrate_langevin_flow_step_one(const azp_flow_method_args* args, void* stream);
int azp_integrate_langevin_flow_step_two(const azp_flow_method_args* args, void* stream);
/* Step two of one time step (at args->timestep) and step one of the next in one kernel, bit-identical to the two
 * calls (as azp_integrate_nve_step_two_one). */
int azp_integrate_langevin_flow_step_two_one(const azp_flow_method_args* args, void* stream);
int azp_integrate_brownian_flow_step(const azp_flow_method_args* args, void* stream);

/* ---- Langevin and Brownian dynamics with rotation (azplugins_amd.methods.Langevin / .Brownian) ----
 * Names and parameters are hoomd.md.methods'; HOOMD-blue's source is not available to this project, so the scheme is
 * DEFINED HERE and pinned by tests/langevin_ref.py. One thread per particle does its translation and,
 * where `rotational` is set, its rotation in the same pass.
 *
 * Translation: exactly the flow methods above at u = 0 and noiseless = 0 (the same device functions, ids 202 / 201,
 * draws k = 0, 1, 2), bit for bit.
 *
 * Rotation. q = d_orientation (scalar first), p = d_angmom, I = d_inertia (N x 3), tau = d_net_torque (N x 4, space
 * frame); body(tau) = rotate(conj(q), tau); S = vec(1/2 conj(q) p) the body angular momentum; an axis k with I_k == 0
 * is not integrated. g_k = d_gamma_r[3 type + k]; R_k = -c_k + 2 c_k u01 with c_k = sqrt(6 g_k kT / dt), draw k + 3 of
 * the translation's key.
 *   Langevin step two (q at t + dt, p at the half step, tau the new torque):
 *     b_k = R_k - g_k S_k / I_k (0 where I_k == 0), stored in d_langevin_torque (N x 4: b_x, b_y, b_z, 0; body frame);
 *     T = body(tau) + b with the components of axes without inertia zeroed; p += dt q (0, T) -- the half kick of
 *     azp_integrate_nve_rot_step_two.
 *   Langevin step one: T = body(tau) + b as stored by the previous step two (zeros before the first); p += dt q (0, T);
 *     free rotations about axes 3, 2, 1, 2, 3; q renormalised -- as azp_integrate_nve_rot_step_one.
 *   The Langevin torque of step two is used again by the next step one, as the Langevin force is in the acceleration:
 *   for a planar rotor without torque the full-step variance of S_z is then exactly kT I_z. With every
 *   g_k = 0 the rotational half is the NVE one bit for bit.
 *   Brownian step (id 201, draws 3..5), on the axes with I_k != 0:
 *     dtheta_k = (body(tau)_k + R_k) dt / g_k (0 where I_k == 0); with |dtheta| > 0
 *     q <- normalize(q (cos(|dtheta| / 2), sin(|dtheta| / 2) dtheta / |dtheta|)), the exponential map in the body frame;
 *     with |dtheta| == 0 q is left as it is. p is not read or written, as the velocities are not.
 * Rows are selected as by the flow methods (type < ntypes, d_type_mask); a row that is not selected keeps every bit.
 * `timestep`, `kT`: of the step that step two (the Brownian step) belongs to; step one draws nothing.
 * N == 0 returns success. AZP_ERROR_INVALID_ARGUMENT: a null pointer that the call needs (d_pos always; d_net_force,
 * d_tag, d_gamma where a step two or a Brownian step runs; d_vel, d_accel for Langevin; with `rotational` d_orientation,
 * d_inertia, d_net_torque, for Langevin d_angmom and d_langevin_torque too, and d_gamma_r where draws are made),
 * ntypes == 0, dt <= 0, a block size other than 0 (256), 64, 128, 192, 256. */
typedef struct azp_langevin_args
    {
    double* d_pos;              /* N x 4 (type in w is preserved) */
    double* d_vel;              /* N x 4 (vx, vy, vz, mass); Langevin only */
    double* d_accel;            /* N x 4 (ax, ay, az, 0); Langevin only */
    const double* d_net_force;  /* N x 4 */
    int32_t* d_image;           /* N x 3 periodic image counters, may be NULL */
    const uint32_t* d_tag;      /* N */
    const double* d_gamma;      /* ntypes friction coefficients */
    const uint8_t* d_type_mask; /* ntypes bytes, may be NULL (every type) */
    double* d_orientation;      /* N x 4 */
    double* d_angmom;           /* N x 4; Langevin only */
    const double* d_inertia;    /* N x 3 */
    const double* d_net_torque; /* N x 4 */
    double* d_langevin_torque;  /* N x 4 (b_x, b_y, b_z, 0), body frame; Langevin only */
    const double* d_gamma_r;    /* ntypes x 3 rotational friction coefficients */
    azp_box box;
    double dt;
    double kT;                  /* kT at `timestep` */
    uint64_t timestep;
    uint32_t seed;              /* low 16 bits used */
    uint32_t rotational;        /* 0: the rotational pointers are not read */
    uint32_t N;
    uint32_t ntypes;
    uint32_t block_size;        /* 0: 256 */
    uint32_t _pad;
    } azp_langevin_args;

int azp_integrate_langevin_step_one(const azp_langevin_args* args, void* stream);
int azp_integrate_langevin_step_two(const azp_langevin_args* args, void* stream);
/* Step two of one time step (at args->timestep) and step one of the next in one kernel, bit-identical to the two calls:
 * q, p, I and the torque are read once. */
int azp_integrate_langevin_step_two_one(const azp_langevin_args* args, void* stream);
int azp_integrate_brownian_step(const azp_langevin_args* args, void* stream);

/* ---- thermostats of the NVE step (azplugins_amd.thermostats: Berendsen, Bussi, MTTK) ----
 * Names and parameter keys are hoomd.md.methods.thermostats'; HOOMD-blue's source is not available to this project,
 * so the scheme is DEFINED HERE and pinned by tests/thermostat_ref.py.
 *
 * A thermostat acts once per step, at the start of step t, on the full-step velocities v(t): it is a scalar map
 * (K, state, t) -> alpha; step one then does v <- alpha v, v += a dt/2, x += v dt, wrap. All N particles.
 *   K    = sum_i 1/2 m_i |v_i|^2, each term 0.5 * (((m vx) vx + (m vy) vy) + (m vz) vz), summed in the reproducible
 *          order of csrc/azp_reduce.hpp
 *   Nf   = `ndof` (the driver passes 3 N - 3), Kbar = Nf kT / 2
 *   Berendsen  alpha = sqrt(1 + (dt / tau) (Kbar / K - 1)); tau >= dt
 *   Bussi      (Bussi, Donadio, Parrinello 2007) c = exp(-dt / tau), c = 0 for tau = 0; R1 standard normal;
 *              S = 2 Gamma((Nf - 1) / 2); K' = (sqrt(c K) + R1 sqrt((1 - c) kT / 2))^2 + (1 - c) (kT / 2) S;
 *              alpha = +sqrt(K' / K)
 *   MTTK       one Nose-Hoover degree of freedom, g(K) = (2 K / (Nf kT) - 1) / tau^2:
 *              xi += (dt / 2) g(K); alpha = exp(-xi dt); eta += xi dt; xi += (dt / 2) g(alpha^2 K)
 *              (the equations xi' = g, eta' = xi, v' = a - xi v)
 *   K == 0     Berendsen and Bussi: alpha = 1, state unchanged; MTTK integrates xi and eta with K = 0
 *   energy     Berendsen and Bussi: the running sum of K - alpha^2 K; MTTK: Nf kT (tau^2 xi^2 / 2 + eta). K + U + energy
 *              is conserved up to the integrator's error
 * Random stream (Bussi): Philox4x32-10 with the flow methods' key layout and id 204, key {204 << 24 |
 * (t >> 32 & 0xff) << 16 | seed, t & 0xffffffff}, counter {k, 0, 0, 0} for draw k, u01 = (u64 >> 11) 2^-53 + 2^-54. A
 * normal is sqrt(-2 ln u_a) cos(2 pi u_b) from two consecutive draws; R1 uses draws 0 and 1. Gamma(a) is Marsaglia and
 * Tsang's with d = a - 1/3, c = 1 / sqrt(9 d): attempt j takes its normal x from draws 2 + 3 j, 3 + 3 j and its uniform
 * u from draw 4 + 3 j; with v = (1 + c x)^3 it returns d v when v > 0 and ln u < x^2 / 2 + d - d v + d ln v; after 32
 * attempts (a guard: the acceptance rate exceeds 0.95 for a >= 1) the value d.
 *
 * d_state: AZP_THERMOSTAT_NSTATE doubles on the device, indexed by the AZP_THERMOSTAT_* slots below; it persists
 * between calls and nothing reads it back. d_partials: azp_thermostat_partials_size(N) bytes.
 *   azp_thermostat_kinetic    d_partials <- the per-workgroup partials of K of d_vel
 *   azp_thermostat_step_two   v += (dt / 2) f / m, and d_partials <- the partials of K of the new v, in one pass
 *   azp_thermostat_advance    folds d_partials (bit for bit the sum reduce_fold gives), computes alpha for the step that
 *                             starts at `timestep`, updates xi / eta / energy and writes alpha, K and the number of
 *                             Gamma attempts to d_state. One wave; kT, tau, dt, ndof, seed, timestep by value
 *   azp_thermostat_step_one   reads alpha from d_state: v = alpha v, v += (dt / 2) f / m, x += dt v, wrap (image counters
 *                             updated) as azp_integrate_nve_step_one does
 * Plain IEEE arithmetic in the order written, no contraction, no atomics. Asynchronous on `stream`.
 * AZP_ERROR_INVALID_ARGUMENT: NULL args, N == 0, a NULL array the call uses, too small a d_partials; for the advance
 * also an unknown kind, dt <= 0, kT <= 0, ndof < 3, tau <= 0 (Bussi: tau < 0), Berendsen with tau < dt. */
typedef enum azp_thermostat_kind
    {
    AZP_THERMOSTAT_BERENDSEN = 0,
    AZP_THERMOSTAT_BUSSI = 1,
    AZP_THERMOSTAT_MTTK = 2
    } azp_thermostat_kind;

#define AZP_THERMOSTAT_NSTATE 8
#define AZP_THERMOSTAT_ALPHA 0    /* the scale factor of the last advance */
#define AZP_THERMOSTAT_K 1        /* the kinetic energy it saw */
#define AZP_THERMOSTAT_ENERGY 2
#define AZP_THERMOSTAT_XI 3       /* MTTK */
#define AZP_THERMOSTAT_ETA 4      /* MTTK */
#define AZP_THERMOSTAT_ATTEMPTS 5 /* Bussi: attempts the Gamma sampler of the last advance took */

typedef struct azp_thermostat_args
    {
    double* d_pos;             /* N x 4 (type in w is preserved); step one */
    double* d_vel;             /* N x 4 (vx, vy, vz, mass) */
    const double* d_net_force; /* N x 4; step one and step two */
    int32_t* d_image;          /* N x 3 periodic image counters, may be NULL; step one */
    double* d_partials;        /* azp_thermostat_partials_size(N) bytes */
    double* d_state;           /* AZP_THERMOSTAT_NSTATE doubles */
    uint64_t partials_bytes;
    azp_box box;
    double dt;
    double kT;                 /* kT at `timestep` */
    double tau;
    double ndof;               /* Nf */
    uint64_t timestep;
    uint32_t seed;             /* low 16 bits used */
    uint32_t kind;             /* azp_thermostat_kind */
    uint32_t N;
    uint32_t _pad;
    } azp_thermostat_args;

int azp_thermostat_partials_size(uint32_t N, uint64_t* bytes);
int azp_thermostat_kinetic(const azp_thermostat_args* args, void* stream);
int azp_thermostat_step_two(const azp_thermostat_args* args, void* stream);
int azp_thermostat_advance(const azp_thermostat_args* args, void* stream);
int azp_thermostat_step_one(const azp_thermostat_args* args, void* stream);

/* ---- barostat (azplugins_amd.ConstantPressure: NPH, and NPT with one of the thermostats above) ----
 * Name and parameter keys are hoomd.md.methods.ConstantPressure's; HOOMD-blue's source is not available to this
 * project, so the scheme is DEFINED HERE and pinned by tests/barostat_ref.py. A Martyna-Tobias-Klein
 * barostat on the three lengths of an orthorhombic box: one rate nu_a per axis a in {x, y, z}, all N particles,
 * translational degrees of freedom. The box itself belongs to the caller (the host), who reads lambda from d_state.
 *
 * Inputs of the advance: d_sums, the 20 doubles of azp_thermo_sums over all particles (K_aa = slots 4, 7, 9; W_aa = slots
 * 10, 13, 15); box.L; S; dt; tauS; Nf = `ndof` (the driver passes 3 N - 3). In this order, plain IEEE, no contraction:
 *   K      = 0.5 ((K_xx + K_yy) + K_zz)
 *   V      = (Lx Ly) Lz
 *   kT_ref = thermostat_kT with a thermostat (d_thermostat_state != NULL). Without one: d_state[REF_KT] if that is > 0,
 *            else (2 K) / Nf, which is then stored in REF_KT (the first advance of a fresh state measures it)
 *   W      = ((Nf + 3) kT_ref) (tauS tauS)
 *   G_a    = (((K_aa + W_aa) - V S_a) + (2 K) / Nf) / W        for an axis whose box_dof bit is set, else 0
 *   couple: the free axes of the coupled set C ({x,y}, {x,z}, {y,z} or {x,y,z}) all take (sum of G_c over C in the order
 *            x, y, z, a frozen axis adding its 0) / (number of free axes in C); AZP_BAROSTAT_COUPLE_NONE: nothing
 *   half update ("close" and "open" alike):  nu_a = nu_a + (0.5 dt) G_a for a free axis; nu_a = 0 for a frozen one
 * phase & AZP_BAROSTAT_CLOSE: one half update. phase & AZP_BAROSTAT_OPEN: one half update, then
 *   trace    = (nu_x + nu_y) + nu_z
 *   alpha_a  = exp(-((nu_a + trace / Nf) (0.5 dt)))
 *   lambda_a = exp(nu_a dt)
 *   b_a      = (dt exp(x)) s(x), x = nu_a (0.5 dt), s(x) = 1 + x2 (1/6 + x2 (1/120 + x2 (1/5040 + x2 (1/362880)))), x2 = x x:
 *              sinh(x) / x, whose truncation is below 2^-53 for |x| <= 0.1
 *   alpha_T  = 1, or with a thermostat the alpha of its advance (the thermostat's scheme above, on d_thermostat_state, with
 *              this K, thermostat_kT / _tau / _kind / _seed, `timestep`, dt and Nf); nu is not thermostatted
 * Close and open in one call are the two half updates one after the other, from the same G: bit for bit what two calls give.
 * Every call then writes ENERGY = (0.5 W) ((nu_x nu_x + nu_y nu_y) + nu_z nu_z), K, V, P_aa = (K_aa + W_aa) / V, W and
 * NONFINITE = 1 if any nu, alpha, lambda or b is not finite (else 0).
 *
 * One step t -> t + dt:
 *   azp_barostat_advance(OPEN)   from the sums of the state at t
 *   the caller reads lambda and multiplies its box lengths by it: args.box of the calls below is the NEW box
 *   azp_barostat_step_one        c_a = alpha_T alpha_a; v_a = c_a v_a; v += ((dt / 2) f) (1 / m);
 *                                r_a = lambda_a r_a + b_a v_a; wrap into the new box (image counters updated) as
 *                                azp_integrate_nve_step_one does; pos.w and vel.w are preserved
 *   the forces at t + dt, with virials (the caller's)
 *   azp_barostat_step_two        v += ((dt / 2) f) (1 / m); v_a = alpha_a v_a
 *   azp_thermo_sums into d_sums, then azp_barostat_advance(CLOSE), in the new box
 * Conserved for S_x = S_y = S_z = S: K + U + S V + ENERGY (+ the thermostat's energy).
 * The step kernels read alpha, lambda, b and alpha_T from d_state. Plain IEEE arithmetic in the order written, no
 * contraction, no atomics. Asynchronous on `stream`.
 * AZP_ERROR_INVALID_ARGUMENT: NULL args, N == 0, a NULL array the call uses (d_image may be NULL), dt <= 0, a tilted box, an
 * edge <= 0, a free axis that is not periodic, box_dof bits above 7; for the advance also tauS <= 0, ndof < 3, an unknown
 * couple code, a phase of 0 or above 3, S not finite, and with a thermostat what azp_thermostat_advance refuses. */
#define AZP_BAROSTAT_NSTATE 24
#define AZP_BAROSTAT_NU 0        /* 0, 1, 2: nu_x, nu_y, nu_z */
#define AZP_BAROSTAT_ALPHA 3     /* 3, 4, 5 */
#define AZP_BAROSTAT_LAMBDA 6    /* 6, 7, 8 */
#define AZP_BAROSTAT_B 9         /* 9, 10, 11 */
#define AZP_BAROSTAT_ALPHA_T 12
#define AZP_BAROSTAT_ENERGY 13
#define AZP_BAROSTAT_V 14        /* the volume the last advance saw */
#define AZP_BAROSTAT_P 15        /* 15, 16, 17: P_xx, P_yy, P_zz it saw */
#define AZP_BAROSTAT_NONFINITE 18
#define AZP_BAROSTAT_REF_KT 19   /* kT_ref of a run without thermostat; 0: not measured yet */
#define AZP_BAROSTAT_K 20        /* the kinetic energy it saw */
#define AZP_BAROSTAT_W 21        /* the barostat's mass W */

#define AZP_BAROSTAT_CLOSE 1u
#define AZP_BAROSTAT_OPEN 2u

typedef enum azp_barostat_couple
    {
    AZP_BAROSTAT_COUPLE_NONE = 0,
    AZP_BAROSTAT_COUPLE_XY = 1,
    AZP_BAROSTAT_COUPLE_XZ = 2,
    AZP_BAROSTAT_COUPLE_YZ = 3,
    AZP_BAROSTAT_COUPLE_XYZ = 4
    } azp_barostat_couple;

typedef struct azp_barostat_args
    {
    double* d_pos;               /* N x 4 (type in w is preserved); step one */
    double* d_vel;               /* N x 4 (vx, vy, vz, mass); step one and step two */
    const double* d_net_force;   /* N x 4; step one and step two */
    int32_t* d_image;            /* N x 3 periodic image counters, may be NULL; step one */
    double* d_state;             /* AZP_BAROSTAT_NSTATE doubles */
    const double* d_sums;        /* AZP_THERMO_NSUMS doubles; the advance */
    double* d_thermostat_state;  /* AZP_THERMOSTAT_NSTATE doubles, or NULL: no thermostat; the advance */
    azp_box box;
    double dt;
    double S[3];                 /* S_xx, S_yy, S_zz */
    double tauS;
    double ndof;                 /* Nf */
    double thermostat_kT;        /* kT at `timestep` */
    double thermostat_tau;
    uint64_t timestep;
    uint32_t thermostat_kind;    /* azp_thermostat_kind */
    uint32_t thermostat_seed;    /* low 16 bits used */
    uint32_t couple;             /* azp_barostat_couple */
    uint32_t box_dof;            /* bit a set: axis a is free */
    uint32_t phase;              /* AZP_BAROSTAT_CLOSE | AZP_BAROSTAT_OPEN */
    uint32_t N;
    } azp_barostat_args;

int azp_barostat_advance(const azp_barostat_args* args, void* stream);
int azp_barostat_step_one(const azp_barostat_args* args, void* stream);
int azp_barostat_step_two(const azp_barostat_args* args, void* stream);

/* ---- energy minimization (azplugins_amd.minimize.FIRE) ----
 * Name and parameter keys are hoomd.md.minimize.FIRE's; HOOMD-blue's source is not available to this project, so the
 * scheme is DEFINED HERE and pinned by tests/fire_ref.py. FIRE (Bitzek et al. 2006) is velocity Verlet
 * whose velocities are steered towards the force and whose time step adapts: the control state, the time step
 * included, lives in d_state on the device and nothing reads it back inside a run. All N particles, translational
 * degrees of freedom only.
 *
 * Sums over all particles, f = d_net_force, v = d_vel, each term in the order written, summed in the reproducible
 * order of csrc/azp_reduce.hpp (partials slot-major in d_partials, slots P, VV, FF, U):
 *   P  = sum ((f.x v.x) + (f.y v.y)) + (f.z v.z)
 *   VV = sum ((v.x v.x) + (v.y v.y)) + (v.z v.z)
 *   FF = sum ((f.x f.x) + (f.y f.y)) + (f.z f.z)
 *   U  = sum f.w   (net_force.w carries each particle's share of the potential energy)
 * Masses do not enter the sums.
 *
 * d_state: AZP_FIRE_NSTATE doubles indexed by the AZP_FIRE_* slots below (unused slots stay 0). Initial values:
 * DT = dt_max, ALPHA = alpha_start, KEEP = 1, MIX = 0, all others 0.
 *
 * One step at timestep t:
 *   1. azp_fire_advance   one wave. Folds the four slots of d_partials (lane l adds the partials l, l + 64, ... in turn
 *        from +0.0, then the butterfly: bit for bit what reduce_fold gives). Then lane 0:
 *          CONVERGED or NONFINITE set: return.
 *          any of the four sums not finite: NONFINITE = 1, KEEP = MIX = 0, return.
 *          store P, VV, FF, U.
 *          N_STEPS >= max(1, min_steps_conv) and sqrt(FF / (3 N)) < force_tol and |U - U_PREV| / N < energy_tol:
 *            CONVERGED = 1, KEEP = MIX = 0, return.
 *          KEEP = 1 - ALPHA; MIX = FF > 0 ? ALPHA * (sqrt(VV) / sqrt(FF)) : 0.
 *          P > 0:  N_POS += 1; if N_POS > min_steps_adapt: DT = min(DT * finc_dt, dt_max), ALPHA = ALPHA * fdec_alpha.
 *          else:   DT = DT * fdec_dt, ALPHA = alpha_start, N_POS = 0, KEEP = MIX = 0 (the velocities are dropped;
 *                  DT has no floor).
 *          U_PREV = U; N_STEPS += 1.
 *   2. azp_fire_step_one  reads DT, KEEP, MIX and the flags from d_state. A flag set: the whole grid returns, nothing
 *        moves. Otherwise v = (KEEP * v) + (MIX * f) per component, v += ((DT / 2) f) (1 / m), x += DT v, wrap (image
 *        counters updated) as azp_integrate_nve_step_one does; pos.w and vel.w are preserved.
 *   3. the forces at t + 1 (the caller's).
 *   4. azp_fire_step_two  reads DT and the flags from d_state (the DT that step one used). A flag set: returns
 *        without writing partials. Otherwise v += ((DT / 2) f) (1 / m) and, in the same pass, d_partials <- the
 *        per-workgroup partials of the four sums of the new v and of f.
 *   azp_fire_measure      d_partials <- the partials of v and f as they stand: the same terms in the same order, no
 *        update, d_state not read. Called once at the start of a run (velocities may have been changed between runs);
 *        after azp_fire_step_two it leaves the same partials bit for bit.
 * Plain IEEE arithmetic in the order written, no contraction, no atomics. Asynchronous on `stream`.
 * AZP_ERROR_INVALID_ARGUMENT: NULL args, N == 0, a NULL array the call uses (d_image may be NULL), a d_partials smaller
 * than azp_fire_partials_size(N); for the advance also dt_max <= 0, force_tol <= 0, energy_tol <= 0, finc_dt <= 1,
 * fdec_dt, alpha_start or fdec_alpha outside (0, 1), or any of them not finite. */
#define AZP_FIRE_NSTATE 16
#define AZP_FIRE_DT 0         /* the time step of the next step one */
#define AZP_FIRE_ALPHA 1
#define AZP_FIRE_KEEP 2       /* the two velocity coefficients of the next step one */
#define AZP_FIRE_MIX 3
#define AZP_FIRE_N_POS 4      /* steps since the last non-positive power */
#define AZP_FIRE_N_STEPS 5    /* advances since reset */
#define AZP_FIRE_U 6          /* the sums the last advance saw */
#define AZP_FIRE_U_PREV 7
#define AZP_FIRE_P 8
#define AZP_FIRE_VV 9
#define AZP_FIRE_FF 10
#define AZP_FIRE_CONVERGED 11
#define AZP_FIRE_NONFINITE 12
#define AZP_FIRE_NSLOTS 4     /* slots of d_partials: P, VV, FF, U */

typedef struct azp_fire_args
    {
    double* d_pos;             /* N x 4 (type in w is preserved); step one */
    double* d_vel;             /* N x 4 (vx, vy, vz, mass) */
    const double* d_net_force; /* N x 4 (fx, fy, fz, energy) */
    int32_t* d_image;          /* N x 3 periodic image counters, may be NULL; step one */
    double* d_partials;        /* azp_fire_partials_size(N) bytes */
    double* d_state;           /* AZP_FIRE_NSTATE doubles */
    uint64_t partials_bytes;
    azp_box box;
    double dt_max;
    double force_tol;
    double energy_tol;
    double finc_dt;
    double fdec_dt;
    double alpha_start;
    double fdec_alpha;
    uint32_t min_steps_adapt;
    uint32_t min_steps_conv;
    uint32_t N;
    uint32_t _pad;
    } azp_fire_args;

int azp_fire_partials_size(uint32_t N, uint64_t* bytes);
int azp_fire_measure(const azp_fire_args* args, void* stream);
int azp_fire_step_two(const azp_fire_args* args, void* stream);
int azp_fire_advance(const azp_fire_args* args, void* stream);
int azp_fire_step_one(const azp_fire_args* args, void* stream);

/* ---- type updates: region type updater and particle evaporator ----
 * The reference's evaporation tools (HOOMD-2-era sources that its CMake no longer builds), restated. Both calls are
 * asynchronous on `stream`, touch rows [0, N) only (ghost rows follow their owner at the next exchange) and write
 * nothing but the type word (low 32 bits) of pos.w: x, y, z keep their bits. A particle ON a face of the slab is
 * inside: inside = !(z > z_hi || z < z_lo).
 *
 * azp_type_update_region (src/TypeUpdater.cc:93-127): every row whose type is inside_type or outside_type gets
 * inside_type if it is inside the slab, else outside_type; rows of other types are untouched. */
typedef struct azp_type_update_args
    {
    double* d_pos;          /* N x 4 */
    uint32_t N;
    uint32_t inside_type;
    uint32_t outside_type;
    uint32_t block_size;    /* 0: 256 */
    double z_lo, z_hi;
    } azp_type_update_args;

int azp_type_update_region(const azp_type_update_args* args, void* stream);

/* azp_evaporate (src/ParticleEvaporator.cc:100-260), one call, no host round trip inside it:
 *   candidates: rows of solvent_type inside the slab (:176-203), M of them;
 *   key of a candidate: u64 = c0 << 32 | tag, c0 the first output word of Philox4x32-10 with counter {0, tag, 0, 0}
 *     and key {203 << 24 | (timestep >> 32 & 0xff) << 16 | seed & 0xffff, timestep & 0xffffffff}: draw 0 of the flow
 *     methods' stream layout with the reference's evaporator id (src/RNGIdentifiers.h). Tags are unique, so are keys;
 *   selection: the min(Nmax, M) candidates with the smallest keys (M < Nmax: all of them, :110-116;
 *     Nmax = 0xffffffff: no limit);
 *   apply: the picked rows get evaporated_type.
 * d_counts (optional): two uint32, M and the number picked.
 *
 * DEPARTURE FROM THE REFERENCE. The reference gathers the candidates' indices in rank order and shuffles them on the
 * host with HOOMD's RandomGenerator / UniformIntDistribution (:229-259). HOOMD's source is not available to this
 * project, so that stream could not be reproduced in any case; and a pick by index changes with the particle sorter
 * and with the number of ranks. The smallest of independent per-tag keys keeps what matters -- every subset of
 * min(Nmax, M) candidates is equally likely, every rank reaches the same result -- and is invariant under
 * re-indexing and under decomposition.
 *
 * Decomposed runs do the same work in two phases: azp_evaporate_local_keys writes this rank's min(Nmax, M) smallest
 * keys in ascending order to d_keys_out (room for min(Nmax, N) keys) and their number to d_n_keys_out (and M, 0 to
 * d_counts); the ranks gather them and take the Nmax-th smallest as the threshold; azp_evaporate_apply_below flips
 * every local candidate whose key is <= threshold_key (d_counts: local candidates, local rows flipped).
 * azp_evaporate is these two with the threshold taken on the device.
 *
 * azp_evaporate (with a limit) and azp_evaporate_local_keys need d_scratch of azp_evaporate_scratch_size(N) bytes;
 * the order of the candidate buffer may differ from call to call, the picked set does not. The selection is an
 * exact most-significant-digit radix select (8-bit digits, integer histograms); no floating-point atomics. */
typedef struct azp_evaporate_args
    {
    double* d_pos;           /* N x 4 */
    const uint32_t* d_tag;   /* N */
    uint32_t N;
    uint32_t solvent_type;
    uint32_t evaporated_type;
    uint32_t Nmax;           /* 0xffffffff: no limit */
    double z_lo, z_hi;
    uint64_t timestep;
    uint32_t seed;           /* low 16 bits used */
    uint32_t block_size;     /* 0: 256 (the passes over the particles; the selection runs 256 wide) */
    void* d_scratch;
    uint64_t scratch_bytes;
    uint32_t* d_counts;      /* 2 x uint32, may be NULL */
    uint64_t* d_keys_out;    /* azp_evaporate_local_keys only */
    uint32_t* d_n_keys_out;  /* azp_evaporate_local_keys only */
    } azp_evaporate_args;

uint64_t azp_evaporate_scratch_size(uint32_t N);
int azp_evaporate(const azp_evaporate_args* args, void* stream);
int azp_evaporate_local_keys(const azp_evaporate_args* args, void* stream);
int azp_evaporate_apply_below(const azp_evaporate_args* args, uint64_t threshold_key, void* stream);

/* ---- box resize: the particles of a box that changes (HOOMD hoomd.update.BoxResize) ----
 * The reference holds no box-resize code; these are HOOMD's documented semantics. One asynchronous launch over rows
 * [0, N), one row per lane, no LDS and no atomics: the result does not depend on the launch shape.
 *
 * A row is SELECTED if d_type_mask is NULL, or if its type t (low 32 bits of pos.w) has t < ntypes and
 * d_type_mask[t] != 0. A selected row is mapped affinely from the old box to the new one, r' = M r, with
 * M = H_new H_old^-1 (H: the lattice vectors as columns, upper triangular) computed by the CALLER in float64 and
 * passed as M = {M00, M01, M02, M11, M12, M22}; the kernel divides nothing and evaluates, in this order,
 *     x' = fma(M02, z, fma(M01, y, M00 * x))
 *     y' = fma(M12, z, M11 * y)
 *     z' = M22 * z
 * (three, two and one roundings). pos.w keeps its bits; velocities are not an argument (HOOMD does not scale them).
 *
 * Then EVERY row, selected or not, is wrapped into `box` (the NEW box) and its image counters (d_image, N x 3, may
 * be NULL) are updated. A selected row keeps its fractional coordinates up to rounding: one shift per axis, the wrap
 * of the integration kernels. An unselected row keeps its position and may lie several images outside a box that has
 * shrunk: it is first taken back by k = rint(f) lattice vectors per periodic axis, f its fractional coordinate in the
 * new box along that axis -- z first (z -= k Lz, y -= k (Lz yz), x -= k (Lz xz), each one FMA with the product in
 * parentheses rounded once), then y from the shifted y and z (y -= k Ly, x -= k (Ly xy)), then x -- and then wrapped
 * with one shift per axis like the others, which settles a row left on a face ([-L/2, L/2)).
 * A non-periodic axis is scaled but not wrapped. The caller keeps the periodic flags of the old box.
 *
 * NULL args, a NULL d_pos, a mask with ntypes == 0, an edge that is not positive and finite, a tilt or an entry of M
 * that is not finite, block_size not a multiple of 64 or above 256: AZP_ERROR_INVALID_ARGUMENT, nothing launched.
 * N == 0: success without a launch. */
typedef struct azp_box_resize_args
    {
    double* d_pos;              /* N x 4 */
    int32_t* d_image;           /* N x 3, may be NULL */
    const uint8_t* d_type_mask; /* ntypes bytes, may be NULL (every row is selected) */
    uint32_t N;
    uint32_t ntypes;            /* entries of d_type_mask */
    uint32_t block_size;        /* 0: 256 */
    uint32_t _pad;
    double M[6];                /* M00, M01, M02, M11, M12, M22 */
    azp_box box;                /* the new box */
    } azp_box_resize_args;

int azp_box_resize(const azp_box_resize_args* args, void* stream);

/* ---- velocity / velocity-field computes ----
 * Replaces the reference's GPU drivers of hoomd.azplugins.compute: the per-particle loop of
 * src/VelocityFieldComputeGPU.cuh:35-71 (CartesianVelocityFieldCompute, CylindricalVelocityFieldCompute) and
 * src/VelocityComputeGPU.cu:48-65 (VelocityCompute = the Cartesian case with num_bins = (0, 0, 0): one bin), with
 * the bins of src/BinningOperation.h, src/CartesianBinningOperation.h and src/CylindricalBinningOperation.h.
 * Rows [0, N) only. A particle is counted if d_type_mask[type] != 0 (d_type_mask NULL: every particle); its
 * position is wrapped into the (global) box, binned as floor(((x - lower) / (upper - lower)) * n) in each
 * dimension with n = num_bins[d] > 0 (outside [0, n) in any: dropped; n = 0: not binned, index 0) and raveled as
 * z + nz (y + ny x) with a dimension that is not binned counting as size 1. Cartesian: (x, y, z) and the momentum
 * m v as it is. Cylindrical: (r, theta, z), theta = atan2(y, x) in [0, 2 pi), the momentum rotated by
 * (cos theta, sin theta) = (x / r, y / r), (1, 0) at r = 0.
 * azp_velocity_field_sums OVERWRITES d_sums (bins x 4: mass, px, py, pz). Deterministic: no floating-point
 * atomics, two calls on the same input give bit-identical sums. It needs a device scratch buffer of at least
 * azp_velocity_field_scratch_size bytes (depends on N and the bin count only).
 * azp_velocity_field_normalize: d_velocity[b] (bins x 3) = momentum / mass, or 0 where the mass is 0
 * (src/VelocityFieldCompute.h:262-278); a decomposed run sums d_sums over its ranks first.
 * Both are asynchronous on `stream`; more than 2^31 - 1 bins: AZP_ERROR_TOO_MANY_BINS; upper <= lower in a
 * binned dimension: AZP_ERROR_INVALID_ARGUMENT. */
typedef enum azp_coordinates
    {
    AZP_COORDINATES_CARTESIAN = 0,
    AZP_COORDINATES_CYLINDRICAL = 1
    } azp_coordinates;

typedef struct azp_velocity_field_args
    {
    const double* d_pos;       /* N x 4 (x, y, z, type bits) */
    const double* d_vel;       /* N x 4 (vx, vy, vz, mass) */
    uint32_t N;
    uint32_t coordinates;      /* azp_coordinates */
    azp_box box;               /* global box */
    uint32_t num_bins[3];      /* Cartesian (x, y, z) or cylindrical (r, theta, z); 0: not binned */
    uint32_t ntypes;           /* entries of d_type_mask */
    double lower[3];
    double upper[3];
    const uint8_t* d_type_mask; /* ntypes bytes, may be NULL */
    double* d_sums;            /* bins x 4, overwritten */
    void* d_scratch;
    uint64_t scratch_bytes;
    } azp_velocity_field_args;

int azp_velocity_field_scratch_size(const azp_velocity_field_args* args, uint64_t* bytes);
int azp_velocity_field_sums(const azp_velocity_field_args* args, void* stream);
int azp_velocity_field_normalize(const double* d_sums, uint64_t n_bins, double* d_velocity, void* stream);

/* ---- thermodynamic sums (compute.ThermodynamicQuantities) ----
 * One deterministic pass over rows [0, N) of a group (d_type_mask[type] != 0 with the type from d_pos[i].w;
 * d_type_mask NULL: every particle, d_pos is then not read) that OVERWRITES the AZP_THERMO_NSUMS doubles at d_out:
 *   0      particle count
 *   1-3    sum m v
 *   4-9    sum m v_a v_b, order xx, xy, xz, yy, yz, zz
 *   10-15  sum of the per-particle virials of every force array with a non-NULL d_virial entry, same order
 *   16     sum of the .w (energy) of every force array
 *   17     sum_k s_k^2 / (2 I_k) over the axes with I_k != 0, s = 1/2 conj(q) p (rotational kinetic energy)
 *   18     number of non-zero inertia components
 *   19     0
 * Slots 17 and 18 are 0 unless d_orientation, d_angmom and d_inertia are given (all three or none). d_out is any
 * device address (8-byte aligned), e.g. a row of a larger table. No floating-point atomics: two calls on the same
 * input give bit-identical rows, and no term passes through more than 200 additions for N <= 2^24
 * (csrc/thermo.hip). Asynchronous on `stream`; needs a device scratch buffer of azp_thermo_scratch_size bytes
 * (depends on N only). AZP_ERROR_INVALID_ARGUMENT: more than AZP_THERMO_MAX_FORCES forces, a NULL d_vel, d_out or
 * listed force array, only some of the three rotational arrays, a mask without d_pos, too small a scratch. */
#define AZP_THERMO_NSUMS 20
#define AZP_THERMO_MAX_FORCES 8

typedef struct azp_thermo_args
    {
    const double* d_vel;         /* N x 4 (vx, vy, vz, mass) */
    const double* d_pos;         /* N x 4, read for the type only; may be NULL without a mask */
    const uint8_t* d_type_mask;  /* ntypes bytes, may be NULL */
    const double* d_force[AZP_THERMO_MAX_FORCES];  /* n_forces arrays, N x 4 */
    const double* d_virial[AZP_THERMO_MAX_FORCES]; /* per force: 6 rows of pitch N, or NULL (no virial) */
    const double* d_orientation; /* N x 4, may be NULL */
    const double* d_angmom;      /* N x 4, may be NULL */
    const double* d_inertia;     /* N x 3, may be NULL */
    double* d_out;               /* AZP_THERMO_NSUMS doubles, overwritten */
    void* d_scratch;
    uint64_t scratch_bytes;
    uint32_t N;
    uint32_t ntypes;             /* entries of d_type_mask */
    uint32_t n_forces;
    uint32_t _pad;
    } azp_thermo_args;

int azp_thermo_scratch_size(const azp_thermo_args* args, uint64_t* bytes);
int azp_thermo_sums(const azp_thermo_args* args, void* stream);

/* ---- thermodynamic sums per bin (compute.ThermodynamicField) ----
 * Not part of the reference: the semantics are DEFINED HERE. The particles of rows [0, N) that
 * d_type_mask selects (NULL: every particle) are wrapped into the box and binned exactly as azp_velocity_field_sums
 * bins them (same triple num_bins / lower / upper, same coordinate systems, same arithmetic: csrc/field_bin.hpp; in
 * the cylindrical system only the BIN is cylindrical, every summed quantity stays Cartesian). Per bin the row holds
 * AZP_THERMO_FIELD_NSUMS + ntypes doubles:
 *   0      n, the particle count
 *   1      M = sum m
 *   2-4    P = sum m v
 *   5-10   K = sum m v_a v_b, order xx, xy, xz, yy, yz, zz
 *   11-16  W = sum over the particles of (the per-particle virials of the force arrays with a non-NULL d_virial entry,
 *          added in the order of the arrays starting from +0.0), same order
 *   17     U = sum over the particles of (the .w of the force arrays, added in the same way)
 *   18...  the count per type (types outside [0, ntypes) are counted in slot 0 only): exact integers stored as doubles
 * d_out (n_bins x (AZP_THERMO_FIELD_NSUMS + ntypes) doubles, bin-major, any 8-byte aligned device address) is
 * OVERWRITTEN, the empty bins with +0.0.
 *
 * Three steps. azp_thermo_field_keys writes d_keys[i] = (bin << 32) | d_tag[i] for the N rows (a row that is not
 * counted gets the bin AZP_THERMO_FIELD_NO_BIN, which sorts last). The caller sorts the keys as signed or unsigned
 * 64-bit integers (they are unique and below 2^63) and hands d_sorted_keys and d_order (int64: d_sorted_keys[p] =
 * d_keys[d_order[p]]) to azp_thermo_field_sums, which finds the non-empty bins and sums each of them in a fixed
 * 64-ary tree: the terms of a bin in tag order are padded with +0.0 to a multiple of 64, every run of 64 is replaced
 * by its balanced pairwise sum ((x0 + x1) + (x2 + x3)) + ..., and this repeats until one value remains. The tree is a
 * function of the members of the bin in tag order and of nothing else: not of N, of the other bins or of the order of
 * the rows. The terms are plain IEEE operations, no contraction: p_a = m v_a, K_ab = p_a v_b. No floating-point
 * atomics. The number of kernel launches depends on N alone (ceil(log64 N) tree levels, at least 1); nothing is read
 * back. All calls are asynchronous on `stream`.
 * The scratch (azp_thermo_field_scratch_size bytes: depends on N, ntypes and the bin count) is used by
 * azp_thermo_field_sums alone.
 * AZP_ERROR_TOO_MANY_BINS: more than 2^31 - 1 bins. AZP_ERROR_INVALID_ARGUMENT, before anything is launched or
 * written: NULL args, upper <= lower in a binned dimension, an unknown coordinate system, more than
 * AZP_THERMO_MAX_FORCES forces or a NULL listed force array, a NULL array the call uses, too small a scratch, phases
 * above 3. N == 0: d_out is zeroed. */
#define AZP_THERMO_FIELD_NSUMS 18
#define AZP_THERMO_FIELD_NO_BIN 0x7fffffffu
#define AZP_THERMO_FIELD_HEADS 1u
#define AZP_THERMO_FIELD_LEVELS 2u

typedef struct azp_thermo_field_args
    {
    const double* d_pos;       /* N x 4 (x, y, z, type bits) */
    const double* d_vel;       /* N x 4 (vx, vy, vz, mass) */
    const uint32_t* d_tag;     /* N */
    const uint8_t* d_type_mask; /* ntypes bytes, may be NULL */
    const double* d_force[AZP_THERMO_MAX_FORCES];  /* n_forces arrays, N x 4 */
    const double* d_virial[AZP_THERMO_MAX_FORCES]; /* per force: 6 rows of pitch N, or NULL (no virial) */
    int64_t* d_keys;           /* N, written by azp_thermo_field_keys */
    const int64_t* d_sorted_keys; /* N, read by azp_thermo_field_sums */
    const int64_t* d_order;    /* N, read by azp_thermo_field_sums */
    double* d_out;             /* bins x (AZP_THERMO_FIELD_NSUMS + ntypes), overwritten */
    void* d_scratch;
    uint64_t scratch_bytes;
    azp_box box;               /* global box */
    double lower[3];
    double upper[3];
    uint32_t num_bins[3];      /* Cartesian (x, y, z) or cylindrical (r, theta, z); 0: not binned */
    uint32_t coordinates;      /* azp_coordinates */
    uint32_t N;
    uint32_t ntypes;           /* entries of d_type_mask and per-type count slots */
    uint32_t n_forces;
    uint32_t phases;           /* 0: all of azp_thermo_field_sums. For timing alone (tools/thermo_field_probe.py):
                                * AZP_THERMO_FIELD_HEADS runs the segment heads only, AZP_THERMO_FIELD_LEVELS zeroes d_out
                                * and runs the tree on the heads that an earlier call left in the scratch */
    } azp_thermo_field_args;

int azp_thermo_field_scratch_size(const azp_thermo_field_args* args, uint64_t* bytes);
int azp_thermo_field_keys(const azp_thermo_field_args* args, void* stream);
int azp_thermo_field_sums(const azp_thermo_field_args* args, void* stream);

/* ---- radial distribution function (compute.RadialDistributionFunction) ----
 * Not part of the reference (azplugins had analyze.rdf in its HOOMD-2 line): the semantics are DEFINED HERE
 * (DESIGN 4.14). For two groups A and B (d_type_mask_a / d_type_mask_b: one byte per type, NULL = every particle; the
 * groups may overlap) in a 3-D box, counts[k] is the number of ORDERED pairs (i in A, j in B, i != j), i over rows
 * [0, N), j over rows [0, n_total) (ghost rows count as partners, never as i), whose minimum-image distance r lies in
 * bin k of num_bins equal bins on [0, r_max):
 *   the pair counts iff rsq < r_max * r_max (the lower edge of a bin is inclusive, r == r_max is excluded);
 *   r = sqrt(rsq), the correctly rounded FP64 square root; k = min((uint32_t)(r * scale), num_bins - 1);
 *   scale = num_bins / r_max is computed once by the caller in double and passed in;
 *   the minimum image is the one the force kernels use (triclinic boxes included).
 * azp_rdf_counts OVERWRITES the num_bins + 4 uint64 at d_out (uninitialised memory is fine, the call zeroes the row
 * on the stream): the counts, then N_A, N_B and N_(A and B) over rows [0, N), then one zero (the word that
 * azp_rdf_subtract_excluded below counts in). From these,
 * g[k] = counts[k] V / (n_pairs (4 pi / 3)(r_(k+1)^3 - r_k^3)) with n_pairs = N_A N_B - N_(A and B)
 * (compute.rdf_from_counts). Integer accumulation only (LDS integer atomics, then 64-bit integer atomic adds): two
 * calls on the same state give the same bits. Asynchronous on `stream`, no host synchronisation, no readback.
 * path: 0 = automatic (the cells wherever they are valid), 1 = all-pairs (any box, O(N_A n_total)), 2 = cells
 * (orthorhombic box with at least three cells of width >= r_max on every periodic axis; a non-periodic axis has
 * clamped cells as azp_cell_grid.periodic = 0); both give the same integers. d_scratch: azp_rdf_scratch_size bytes
 * (depends on n_total, box, r_max and path; 0 for all-pairs, then d_scratch may be NULL).
 * AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written: r_max <= 0, num_bins < 1 or > AZP_RDF_MAX_BINS,
 * scale <= 0, r_max larger than half the smallest perpendicular width of a periodic axis (the minimum image would not
 * be unique), path = 2 where the cells are not valid (never silently replaced), N > n_total, a NULL d_out, too small a
 * scratch. */
#define AZP_RDF_MAX_BINS 8192

typedef struct azp_rdf_args
    {
    const double* d_pos;          /* n_total x 4 (x, y, z, type bits) */
    uint32_t N;                   /* rows that count as i */
    uint32_t n_total;             /* rows that count as j (N + ghosts) */
    azp_box box;                  /* global box */
    uint32_t ntypes;              /* entries of the masks */
    uint32_t num_bins;
    const uint8_t* d_type_mask_a; /* ntypes bytes, may be NULL */
    const uint8_t* d_type_mask_b; /* ntypes bytes, may be NULL */
    double r_max;
    double scale;                 /* num_bins / r_max */
    uint32_t path;                /* 0 auto, 1 all-pairs, 2 cells */
    uint32_t _pad;
    uint64_t* d_out;              /* num_bins + 4, overwritten */
    void* d_scratch;
    uint64_t scratch_bytes;
    } azp_rdf_args;

int azp_rdf_scratch_size(const azp_rdf_args* args, uint64_t* bytes);
int azp_rdf_counts(const azp_rdf_args* args, void* stream);

/* Intermolecular g(r): take the excluded pairs (a table of neighbor-list exclusions: entry s of row i is
 * d_excl[s * excl_pitch + i], s < d_n_excl[i], i < N; symmetric, free of duplicates and of self-entries) out of a row
 * that azp_rdf_counts has filled for `rdf` (the same arguments, the same d_out), queued on the same stream after it.
 * One lane per row i walks the row's entries j; where i is in A and j in B the pair goes through the arithmetic of the
 * main pass (the bin of a pair is a function of its rsq alone, so it is the bin the pair was counted in; a pair at
 * rsq >= r_max^2 was not counted and is not subtracted) into an integer histogram of the workgroup, which is then
 * SUBTRACTED from the row: 2^64 - v added with the 64-bit integer atomic. d_out[num_bins + 3], which azp_rdf_counts
 * leaves zero, receives the number of ORDERED pairs subtracted. Integers only: two calls give the same bits. N_A, N_B
 * and N_(A and B), and with them the normalisation n_pairs, stay as they are. An entry j >= n_total is skipped.
 * Rows that sit on the rank twice (a particle and its own periodic ghost) are not handled: single-domain states only.
 * AZP_ERROR_INVALID_ARGUMENT: what azp_rdf_counts refuses, a NULL table, excl_pitch < N. N == 0: success. */
typedef struct azp_rdf_exclusion_args
    {
    azp_rdf_args rdf;           /* as given to azp_rdf_counts; path, d_scratch and scratch_bytes are not looked at */
    const uint32_t* d_n_excl;   /* N */
    const uint32_t* d_excl;     /* width x excl_pitch */
    uint64_t excl_pitch;
    } azp_rdf_exclusion_args;

int azp_rdf_subtract_excluded(const azp_rdf_exclusion_args* args, void* stream);

/* ---- distributions of the bonded coordinates (compute.BondedDistribution) ----
 * Not part of the reference; the semantics are DEFINED HERE. One histogram per group type of the bond
 * lengths, the bending angles or the dihedral angles of a state: what a tabulated bonded potential is inverted from.
 * The groups come from the per-particle table of their kind (the one the force kernels walk; arity 2 is the layout of
 * the bond table, which the special pairs share): one lane per row i < N walks its entries and counts those in which
 * i is member 0 of the group, so every group with its first member on a row below N is counted exactly once (on a
 * decomposed run every particle is a local row of exactly one rank). An entry whose type is >= n_types or which
 * names a row >= n_max is skipped. The coordinate x of a group, separations by the minimum image of the force kernels:
 *   arity 2   r = sqrt(|r_a - r_b|^2), correctly rounded, on [lo, hi) = [r_min, r_max): a group with r < r_min or
 *             r >= r_max (or a NaN) goes to the `outside` word of its type
 *   arity 3   theta = atan2(|dab x dcb|, dab . dcb) with dab = r_a - r_b, dcb = r_c - r_b, on [0, pi]: well
 *             conditioned at 0 and pi, where acos is not
 *   arity 4   phi = atan2(|b2| (b1 . n2), n1 . n2) on [-pi, pi], b1, b2, b3, n1, n2 as for the dihedral forces (the
 *             common positive factor 1 / (|n1||n2|) of the force kernel's sin phi and cos phi is left out: atan2
 *             does not see it)
 *   bin       k = min((uint32_t)((x - lo) * scale), num_bins - 1), scale = num_bins / (hi - lo) in double, pi = M_PI:
 *             lower edges are inclusive, theta == pi and phi == pi fall into the last bin.
 * d_out: n_types * (num_bins + 2) uint64, per type counts[num_bins], then `outside`, then `total` = every group of the
 * type that was looked at (the sum of the counts and of `outside`). The call OVERWRITES the row (it zeroes it on the
 * stream first; uninitialised memory is fine), so a recorder can point it at a row of its table. Integers only:
 * a uint32 histogram of the workgroup in LDS (integer LDS atomics), flushed into the row with 64-bit integer atomic
 * adds on its non-zero words, and `total` summed from the finished row by a second small launch on the same stream;
 * two calls give the same bits. No forces and no force parameters are read or written.
 * path: 0 = automatic, 1 = the LDS histogram, 2 = 64-bit integer atomics straight on the row. The histogram of a
 * workgroup is n_types * (num_bins + 2) words and a workgroup can have 64 KiB of LDS here, so path 1 exists for at
 * most AZP_BONDED_HISTOGRAM_LDS_WORDS = 16384 words; path 0 takes it wherever it exists and path 2 elsewhere. Both
 * give the same integers.
 * AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written: NULL args; arity not 2, 3 or 4; num_bins < 1
 * or > AZP_RDF_MAX_BINS; n_types == 0; path > 2, or 1 where the histogram does not fit; arity 2 without finite
 * 0 <= r_min < r_max. N == 0: success before any array is looked at (a d_out that is given is zeroed, NULL is
 * accepted). Otherwise also: a NULL d_out, d_pos, table or count array (arity 2: a NULL d_table_pos), pitch < N,
 * N > n_max. A NaN coordinate (coincident or collinear members) goes to `outside`. */
#define AZP_BONDED_HISTOGRAM_LDS_WORDS 16384

typedef struct azp_bonded_histogram_args
    {
    const double* d_pos;         /* n_max x 4 */
    uint32_t N;                  /* rows whose entries are walked */
    uint32_t n_max;              /* rows an entry may name (N + ghosts) */
    azp_box box;
    uint32_t arity;              /* 2: bonds and special pairs, 3: angles, 4: dihedrals */
    uint32_t n_types;
    const void* d_table;         /* azp_bond_entry / azp_angle_entry / azp_dihedral_entry at [s * pitch + i] */
    const uint32_t* d_table_pos; /* arity 2: the row's position in the group, [s * pitch + i] */
    const uint32_t* d_counts;    /* N */
    uint64_t pitch;
    uint32_t num_bins;
    uint32_t path;               /* 0 auto, 1 LDS histogram, 2 global atomics */
    double r_min, r_max;         /* arity 2; ignored otherwise */
    uint64_t* d_out;             /* n_types * (num_bins + 2), overwritten */
    } azp_bonded_histogram_args;

int azp_bonded_histogram(const azp_bonded_histogram_args* args, void* stream);

/* ---- static structure factor (compute.StructureFactor) ----
 * Not part of the reference; the semantics are DEFINED HERE. For a 3-D box periodic on all three axes with
 * lattice matrix H (columns a_1 = (Lx, 0, 0), a_2 = (xy Ly, Ly, 0), a_3 = (xz Lz, yz Lz, Lz)) the wavevectors are
 * q(m) = 2 pi H^-T m for integer triples m = (h, k, l), so that q . r = 2 pi m . f with f the coordinates along the
 * lattice vectors (f in [-0.5, 0.5) for a wrapped particle; csrc/cell_bin.hpp fractional()). For two groups A and B
 * (d_type_mask_a / d_type_mask_b: one byte per type, NULL = every particle; the groups may overlap) the amplitude of a
 * group is
 *   rho_G(m) = sum over rows j < N of G of exp(-2 pi i m . f_j)           (ghost rows, >= N, are never read)
 * and the partial structure factor (Ashcroft-Langreth) S_AB(m) = Re[rho_A(m) conj(rho_B(m))] / sqrt(N_A N_B)
 * (compute.structure_factor_from_amplitudes). Which vectors, and how S_AB(m) is averaged over |q|, is the caller's
 * matter (compute.StructureFactor: one of each +-pair with |q| < q_max, order (l, k, h)).
 * azp_structure_factor_amplitudes OVERWRITES the 4 n_vectors + 4 doubles at d_out (uninitialised memory is fine):
 * Re rho_A[0 .. n), Im rho_A[0 .. n), Re rho_B[0 .. n), Im rho_B[0 .. n), then N_A, N_B, N_(A and B) over rows [0, N)
 * and one zero. same_groups != 0: B is A (d_type_mask_b is not looked at), the B half is the copy of the A half and is
 * computed once. Asynchronous on `stream`, no host synchronisation, no readback.
 * path: 1 = direct, t = h f_x + k f_y + l f_z and sincospi(2 t) per (particle, vector); 2 = powers, the term is the
 * product e_x^h e_y^k e_z^l of per-particle tables in LDS that are built by repeated complex multiplication from the
 * three base phasors sincospi(2 f) -- it needs m_max, the caller's bound of |h|, |k|, |l| over the vectors, and exists
 * where 32 (m_max[0] + m_max[1] + m_max[2] + 3, made odd) 16 <= AZP_SF_POWERS_LDS_BYTES, i.e. a sum of at most 92; 0 = automatic: THE POWERS
 * PATH WHEREVER IT EXISTS, the direct path elsewhere (the powers path was the faster one at every probed shape at
 * which it exists: profiles/structure_factor.md). Both paths add the same terms in the same order.
 * Order of summation: no floating-point atomics, every order is fixed by N and n_vectors alone, two calls on one
 * state give the same bits. One lane owns one vector; a workgroup takes a chunk of `stages` stages of 256 particles; a
 * lane adds the terms of a stage in row order to a stage accumulator (from +0.0), the stage accumulators in turn to its
 * chunk accumulator (from +0.0); the n_chunks chunk sums of a (vector, slot) are folded as csrc/azp_reduce.hpp does
 * (lane l of one wave adds the partials l, l + 64, ... in turn, then the butterfly). With
 * target = clamp(4096 / ceil(n_vectors / 256), 16, 512): stages = max(1, ceil(ceil(N / 256) / target)), n_chunks =
 * max(1, ceil(ceil(N / 256) / stages)). ADDITION DEPTH D = 256 + stages + ceil(n_chunks / 64) + 6 (278 at N = 2^20
 * with up to 2,048 vectors). Error of one amplitude component: at most N_G 2^-52 (c_arg |m|_1 + c_trig + D) with
 * c_arg = pi (e_f + 1.5), e_f the rounding of fractional() in units of 2^-53 (1 in an orthorhombic box: c_arg = 7.9; it
 * grows with the tilts and the aspect ratio), and c_trig = 4 (derived in tests/structure_factor_ref.py).
 * d_scratch: azp_structure_factor_scratch_size bytes, (n_slots n_vectors + 3) n_chunks doubles with n_slots = 2 for
 * same_groups and 4 otherwise.
 * AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written: NULL args; n_vectors == 0 or >
 * AZP_SF_MAX_VECTORS; a non-periodic axis; a box length that is not positive and finite; path > 2, or 2 where the
 * tables do not fit (never silently replaced); a mask with ntypes == 0; a NULL d_out or d_vectors; with N > 0 a NULL
 * d_pos or too small a scratch. N == 0: success, the row is zeroed. With path 2 a vector beyond m_max is evaluated at
 * the clamped index (a wrong amplitude, no wild read). */
#define AZP_SF_MAX_VECTORS 65536
#define AZP_SF_POWERS_LDS_BYTES 49152
#define AZP_SF_PATH_AUTO 0
#define AZP_SF_PATH_DIRECT 1
#define AZP_SF_PATH_POWERS 2

typedef struct azp_structure_factor_args
    {
    const double* d_pos;          /* N x 4 at least (x, y, z, type bits) */
    uint32_t N;                   /* owned rows */
    uint32_t ntypes;              /* entries of the masks */
    azp_box box;                  /* global box, periodic on all three axes */
    const uint8_t* d_type_mask_a; /* ntypes bytes, may be NULL */
    const uint8_t* d_type_mask_b; /* ntypes bytes, may be NULL */
    uint32_t same_groups;         /* B is A: computed once, copied */
    uint32_t n_vectors;           /* 1 .. AZP_SF_MAX_VECTORS */
    const int32_t* d_vectors;     /* n_vectors x 3 (h, k, l), device memory */
    uint32_t m_max[3];            /* bound of |h|, |k|, |l| over d_vectors (the powers path sizes its tables by it) */
    uint32_t path;                /* 0 auto, 1 direct, 2 powers */
    double* d_out;                /* 4 n_vectors + 4, overwritten */
    void* d_scratch;
    uint64_t scratch_bytes;
    } azp_structure_factor_args;

int azp_structure_factor_scratch_size(const azp_structure_factor_args* args, uint64_t* bytes);
int azp_structure_factor_amplitudes(const azp_structure_factor_args* args, void* stream);

/* ---- bond-orientational order (compute.Steinhardt, compute.SolidLiquid) ----
 * Not part of the reference; the semantics are DEFINED HERE. Steinhardt's q_l, Lechner and Dellago's
 * neighbour average and ten Wolde and Frenkel's solid-bond count, for the rows [0, N) of a 3-D box.
 * Group and neighbours: G = the rows whose type has a non-zero byte in d_type_mask (NULL: every row). The neighbours of
 * i in G are the j in G, j != i, with rsq < r_max * r_max, where (dx, dy, dz) = r_i - r_j goes through the minimum image
 * of the force kernels and rsq = dx dx + dy dy + dz dz: the acceptance rule of azp_rdf_counts. N_b(i) is their number,
 * 0 for a row outside G. The bond is r_ij = -(dx, dy, dz), from i to j.
 * First pass: for term t (l = l[t]) and m = 0 .. l
 *   S_lm(i) = sum over the neighbours j of ( llrint(Re Y_lm(r_ij) 2^40), llrint(Im Y_lm(r_ij) 2^40) )   two int64
 * with the orthonormal Y_lm in the Condon-Shortley phase; Y_l,-m = (-1)^m conj(Y_lm) is never stored. A row owns
 * `words` = sum_t 2 (l[t] + 1) int64: term t from offset sum_{s<t} 2 (l[s] + 1), component m at + 2 m (Re), + 2 m + 1
 * (Im, 0 for m = 0). Y_lm = N_lm Q_l^m(z / r) ((x + i y) / r)^m with r = sqrt(rsq) and IEEE quotients, Q_l^m = P_l^m /
 * (1 - z^2)^(m / 2) by the upward recurrence Q_m^m = (-1)^m (2m - 1)!!, (l + 1 - m) Q_(l+1)^m = (2l + 1) z Q_l^m -
 * (l + m) Q_(l-1)^m (csrc/steinhardt_device.hpp: no trigonometry, no pole). norm[t][m] = N_lm = sqrt((2l + 1) / (4 pi)
 * (l - m)! / (l + m)!) comes from the caller. A bond with rsq == 0 counts in N_b and adds no term. The sums are
 * integers: they do not depend on the order of the additions, two calls give the same bits on either path, and a
 * particle keeps its words when the rows are re-ordered. |Y| <= 1.41 and N <= 2^21 keep |S| below 2^62.
 * Finish: q_lm(i) = double(S_lm) 2^-40 / N_b(i), 0 where N_b == 0; q_l(i) = sqrt(4 pi / (2l + 1) (|q_l0|^2 +
 * 2 sum_{m>0} |q_lm|^2)), added in the order m = 0, 1, ...
 * AZP_STEINHARDT_AVERAGE: T_lm(i) = sum over k in {i} and the neighbours of i of llrint(q_lm(k) 2^40) for i in G (0
 * elsewhere), qbar_lm = double(T) 2^-40 / (N_b(i) + 1), qbar_l from qbar_lm as q_l from q_lm.
 * AZP_STEINHARDT_CONNECTIONS (n_terms == 1): with |q(i)| = sqrt(sum_{m=-l..l} |q_lm(i)|^2),
 *   d(i, j) = Re sum_{m=-l..l} q_lm(i) conj(q_lm(j)) / (|q(i)| |q(j)|)
 * the bond to neighbour j is solid iff d > q_threshold, never where either norm is 0; num_connections(i) is their
 * number and i is solid iff i is in G and num_connections(i) >= solid_threshold.
 * Outputs, all OVERWRITTEN (uninitialised memory is fine), per row of [0, N): d_num_neighbors, d_words (S), d_order
 * (n_terms doubles: q_l, or qbar_l with AVERAGE; 0 outside G), d_avg_words (T, AVERAGE only), d_num_connections
 * (CONNECTIONS only). d_summary: 4 + n_terms (1 + num_bins) + 33 int64, written by the last kernel with 64-bit integer
 * atomics: N_G; the number of rows of G with N_b > 0; sum of N_b; N_solid (0 without CONNECTIONS); per term
 * sum_{i in G} llrint(d_order 2^40); per term a histogram of d_order over G in num_bins bins on [0, 1], k =
 * min((uint32_t)(q num_bins), num_bins - 1); 33 words of histogram of num_connections over G, the last for >= 32
 * (zeros without CONNECTIONS).
 * path: 0 = automatic (the cells wherever they are valid), 1 = all-pairs (any box), 2 = cells (orthorhombic box with at
 * least three cells of width >= r_max on every periodic axis, the grid rule of azp_rdf_counts). Both give the same
 * integers. The particles are binned by the counting sort of the neighbor list in the call's own scratch; candidates
 * are staged through LDS; every accumulation is integer (LDS 64-bit integer atomics); no floating-point atomics.
 * Asynchronous on `stream`: nothing is read back, nothing synchronises. d_scratch: azp_steinhardt_scratch_size bytes.
 * AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written: NULL args; r_max not positive and finite;
 * n_terms outside 1 .. AZP_STEINHARDT_MAX_TERMS; an l outside 1 .. AZP_STEINHARDT_MAX_L or given twice; a norm outside
 * (0, 2); unknown flags; CONNECTIONS with n_terms != 1 or a q_threshold that is not finite; num_bins outside 1 ..
 * AZP_STEINHARDT_MAX_BINS; N > 2^21; a box length that is not positive; r_max larger than half the perpendicular width
 * of a periodic axis; path > 2, or 2 where the cells are not valid (never silently replaced); a mask with ntypes == 0;
 * a NULL output that the flags ask for; with N > 0 a NULL d_pos or too small a scratch. N == 0: the summary is zeroed. */
#define AZP_STEINHARDT_MAX_TERMS 4
#define AZP_STEINHARDT_MAX_L 12
#define AZP_STEINHARDT_MAX_BINS 1024
#define AZP_STEINHARDT_MAX_N (1u << 21)
#define AZP_STEINHARDT_AVERAGE 1u
#define AZP_STEINHARDT_CONNECTIONS 2u
#define AZP_STEINHARDT_CONNECTION_BINS 33

typedef struct azp_steinhardt_args
    {
    const double* d_pos;          /* N x 4 (x, y, z, type bits) */
    uint32_t N;
    uint32_t ntypes;              /* entries of the mask */
    azp_box box;
    const uint8_t* d_type_mask;   /* ntypes bytes, may be NULL */
    double r_max;
    double q_threshold;           /* CONNECTIONS */
    uint32_t solid_threshold;     /* CONNECTIONS */
    uint32_t n_terms;
    uint32_t l[AZP_STEINHARDT_MAX_TERMS];
    double norm[AZP_STEINHARDT_MAX_TERMS][AZP_STEINHARDT_MAX_L + 1];
    uint32_t flags;
    uint32_t path;                /* 0 auto, 1 all-pairs, 2 cells */
    uint32_t num_bins;
    uint32_t _pad;
    uint32_t* d_num_neighbors;    /* N */
    int64_t* d_words;             /* N x words */
    double* d_order;              /* N x n_terms */
    int64_t* d_avg_words;         /* N x words, AVERAGE */
    uint32_t* d_num_connections;  /* N, CONNECTIONS */
    int64_t* d_summary;           /* 4 + n_terms (1 + num_bins) + 33 */
    void* d_scratch;
    uint64_t scratch_bytes;
    } azp_steinhardt_args;

int azp_steinhardt_scratch_size(const azp_steinhardt_args* args, uint64_t* bytes);
int azp_steinhardt_compute(const azp_steinhardt_args* args, void* stream);

/* ---- clusters (compute.Cluster) ----
 * Not part of the reference; the semantics are DEFINED HERE. The connected components of the graph whose
 * vertices are a group of the rows [0, N) of a 3-D box and whose edges are the pairs closer than r_max.
 * Group: G = the rows whose type has a non-zero byte in d_type_mask (NULL: every row) and, where d_member is not NULL,
 * d_member[i] >= member_min (compute.Cluster(solid=...): d_member = the num_connections of a SolidLiquid, member_min
 * its solid_threshold).
 * Edges: i, j in G, i != j, rsq < r_max * r_max, where (dx, dy, dz) = r_i - r_j goes through the minimum image of the
 * force kernels and rsq = dx dx + dy dy + dz dz: the acceptance rule of azp_rdf_counts and azp_steinhardt_compute.
 * Tilted boxes and non-periodic axes included.
 * Clusters: the connected components. A row of G without an edge is a cluster of size 1.
 * Outputs, all OVERWRITTEN, per row: d_cluster_key[i] = the smallest d_tag among the rows of i's cluster,
 * AZP_CLUSTER_NONE outside G (the key does not depend on the order of the rows: it survives the particle sorter);
 * d_cluster_size[i] = the size of i's cluster, 0 outside G.
 * d_summary: 6 + size_bins int64, exact integers:
 *   [0] N_G   [1] the number of clusters   [2] the size of the largest cluster   [3] the key of the largest cluster,
 *   among equal sizes the smallest key, -1 when N_G == 0   [4] the sum over the clusters of size^2   [5] the number of
 *   edges (accepted pairs counted once)   [6 + s - 1] the number of clusters of size s for s < size_bins, the last
 *   word the number of clusters of size >= size_bins.
 * Reproducibility: a concurrent union-find labels the components in whatever order the hardware takes the pairs;
 * everything the call OUTPUTS is a function of the graph and the tags alone. Two calls, the two paths and a re-ordered
 * state give the same key and size per tag and the same summary. Integer atomics only.
 * path: 0 = automatic (the cells wherever they are valid), 1 = all-pairs (any box), 2 = cells (orthorhombic box with at
 * least three cells of width >= r_max on every periodic axis: the grid rule of azp_steinhardt_compute).
 * stages: 0 = the whole call. 1 and 2 are for timing only and leave the outputs unwritten but for a zeroed summary and
 * (2) its word [5]: 1 stops after the rows are ordered, 2 after the union pass.
 * N <= AZP_CLUSTER_MAX_N = 2^30: slots and AZP_CLUSTER_NONE fit 32 bits with room for the index arithmetic of the
 * walk, and the sum of size^2 stays below 2^60.
 * Asynchronous on `stream`: nothing is read back, nothing synchronises. d_scratch: azp_cluster_scratch_size bytes.
 * AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written: NULL args; r_max not positive and finite;
 * size_bins outside 1 .. AZP_CLUSTER_MAX_BINS; N > AZP_CLUSTER_MAX_N; a box length that is not positive; r_max larger
 * than half the perpendicular width of a periodic axis; path > 2, or 2 where the cells are not valid (never silently
 * replaced); stages > 2; a mask with ntypes == 0; a NULL d_summary; with N > 0 a NULL d_pos, d_tag, d_cluster_key or
 * d_cluster_size or too small a scratch. N == 0: the summary is 0 but for [3] = -1. */
#define AZP_CLUSTER_NONE 0xffffffffu
#define AZP_CLUSTER_MAX_BINS 1024
#define AZP_CLUSTER_MAX_N (1u << 30)

typedef struct azp_cluster_args
    {
    const double* d_pos;          /* N x 4 (x, y, z, type bits) */
    uint32_t N;
    uint32_t ntypes;              /* entries of the mask */
    azp_box box;
    const uint8_t* d_type_mask;   /* ntypes bytes, may be NULL */
    const uint32_t* d_tag;        /* N */
    const uint32_t* d_member;     /* N, may be NULL */
    uint32_t member_min;
    uint32_t path;                /* 0 auto, 1 all-pairs, 2 cells */
    double r_max;
    uint32_t size_bins;           /* 1 .. AZP_CLUSTER_MAX_BINS */
    uint32_t stages;              /* 0: everything */
    uint32_t* d_cluster_key;      /* N */
    uint32_t* d_cluster_size;     /* N */
    int64_t* d_summary;           /* 6 + size_bins */
    void* d_scratch;
    uint64_t scratch_bytes;
    uint32_t* d_cluster_rep;      /* N, may be NULL: the row that represents the row's cluster (below) */
    } azp_cluster_args;

int azp_cluster_scratch_size(const azp_cluster_args* args, uint64_t* bytes);
int azp_cluster_compute(const azp_cluster_args* args, void* stream);

/* ---- cluster properties (compute.ClusterProperties) ----
 * Not part of the reference; the semantics are DEFINED HERE: the centre and the gyration tensor of every
 * cluster of an azp_cluster_compute call that has at least min_size particles. Every particle has weight 1.
 * Inputs: d_pos and box of that call and its outputs d_cluster_key, d_cluster_size and d_cluster_rep.
 * d_cluster_rep (the optional output of azp_cluster_compute, NULL there changes nothing): for a row of the group the
 * index of the ROW that represents its cluster (the row of the union-find's root slot): equal for all rows of a cluster,
 * rep[rep[i]] == rep[i]; AZP_CLUSTER_NONE outside the group. Which row represents a cluster is unspecified. (Tags are
 * not bounded by N, so a key cannot index a table: the representative row can.)
 * With H the lattice matrix (columns (Lx, 0, 0), (xy Ly, Ly, 0), (xz Lz, yz Lz, Lz)), origin = -H (1/2, 1/2, 1/2) and
 * s_i = H^-1 (r_i - origin) the fractional coordinate the tilted cell list bins by, in [0, 1) for a wrapped particle:
 *   reference point  periodic axis k: C_k = sum cos(2 pi s_ik), S_k = sum sin(2 pi s_ik) (sincospi of 2 s),
 *                    s0_k = atan2(S_k, C_k) / (2 pi) brought into [0, 1), 0 where both sums are 0;
 *                    non-periodic axis: s0_k = 1/2
 *   unwrapping       ds_i = s_i - s0, on periodic axes minus rint(ds): |ds| <= 1/2
 *   moments          M1 = sum ds, M2 = sum ds (x) ds, per axis min and max of ds
 *   results          m = M1 / n; centre = origin + H (s0 + m), wrapped into the box on periodic axes;
 *                    G = H (M2 / n - m m^T) H^T; Rg^2 = tr G; extent_k = max ds_k - min ds_k;
 *                    compact = 1 where extent_k < 1/2 on every periodic axis
 * compact == 1 exactly when the cluster, unwrapped along its edges, extends over less than half the box on every
 * periodic axis; centre and G are then exact. Otherwise the same formulas are written: reproducible, their meaning
 * the caller's business (a cluster that wraps round the box is never compact).
 * All sums are integers in units of 2^-shift, shift = min(52, 61 - ceil(log2(max(N, 2)))): every term (|term| <= 1)
 * goes through a round-to-nearest conversion of term * 2^shift and is added with 64-bit integer atomics, so the row of
 * a key is bit-identical between two calls, the two paths of azp_cluster_compute and a re-ordered state.
 * d_table: floor(N / min_size) rows of AZP_CLUSTER_PROPERTIES_ROW = 16 doubles (always enough), in the order of the
 * representatives' rows (unspecified): [0] key [1] size [2..4] centre [5..10] G as xx, xy, xz, yy, yz, zz [11] Rg^2
 * [12] compact [13..15] fractional extents. Rows behind summary [0] are not written.
 * d_summary: AZP_CLUSTER_PROPERTIES_SUMMARY = 20 doubles, OVERWRITTEN: [0] the number of table rows [1] the particles
 * in them [2] shift [3] 0 [4..19] the table row of the largest cluster, among equal sizes the smallest key (as summary
 * [3] of azp_cluster_compute); no rows: zeros with key -1.
 * Asynchronous on `stream`: nothing is read back. d_scratch: azp_cluster_properties_scratch_size bytes.
 * AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written: NULL args; min_size == 0; N > AZP_CLUSTER_MAX_N;
 * a box length that is not positive; a NULL d_summary; with N > 0 a NULL d_pos, d_cluster_rep, d_cluster_key,
 * d_cluster_size, d_table or too small a scratch. */
#define AZP_CLUSTER_PROPERTIES_ROW 16
#define AZP_CLUSTER_PROPERTIES_SUMMARY 20

typedef struct azp_cluster_properties_args
    {
    const double* d_pos;              /* N x 4 */
    uint32_t N;
    uint32_t min_size;                /* >= 1 */
    azp_box box;
    const uint32_t* d_cluster_rep;    /* N */
    const uint32_t* d_cluster_key;    /* N */
    const uint32_t* d_cluster_size;   /* N */
    double* d_table;                  /* floor(N / min_size) x 16 */
    double* d_summary;                /* 20 */
    void* d_scratch;
    uint64_t scratch_bytes;
    } azp_cluster_properties_args;

int azp_cluster_properties_scratch_size(const azp_cluster_properties_args* args, uint64_t* bytes);
int azp_cluster_properties(const azp_cluster_properties_args* args, void* stream);

/* ---- wall potentials (azplugins_amd.wall) ----
 * Replace the reference's legacy wall evaluators src/WallEvaluatorLJ93.h:50-150 and
 * src/WallEvaluatorColloid.h:52-195 with their instantiation src/WallPotentials.h / src/WallPotentials.cu. The two
 * headers define only V(r); the loop over walls, the geometries and the extrapolated mode live in HOOMD's wall code,
 * which is not available to this project, so everything else is DEFINED HERE.
 *
 * A wall yields a signed distance d and a unit vector u (the direction in which d grows); x is the particle position
 * after the wrap into the box that the barrier kernels apply, walls are not periodic (no minimum image):
 *   AZP_WALL_PLANE     d = n.(x - origin), u = n                               (axis = unit normal n)
 *   AZP_WALL_SPHERE    rho = |x - origin|; inside: d = R - rho, u = -(x - origin) / rho; outside: d = rho - R,
 *                      u = (x - origin) / rho; rho == 0: u = 0
 *   AZP_WALL_CYLINDER  s = (x - origin) - ((x - origin).a) a, rho = |s|, then as the sphere with s (axis = unit a)
 * d is computed with IEEE operations in the order written, sums left to right, no contraction, correctly rounded
 * square root, so a host restatement reproduces it bit for bit.
 * With c = r_cut and e = r_extrap of the particle's type, one wall contributes
 *   e == 0:  0 < d < c: E = V(d) - shift, F = -V'(d) u; otherwise nothing (also d <= 0, d == c)
 *   e  > 0:  d >= e as above; d < e (also behind the wall): E = V(e) - shift + F_e (e - d), F = F_e u, F_e = -V'(e)
 * The contributions of the walls are added in list order. The per-particle virial is not defined by the reference's
 * headers: d_virial is set to zero when it is not NULL.
 * d_params: AZP_WALL_PARAM_DOUBLES doubles per type, made by azp_wall_*_params_make:
 *   0, 1  coefficients (Colloid: A sigma^6 / 7560, A / 6; LJ93: epsilon, sigma as given -- folding them would round
 *         them, and near the zero of the force that rounding is amplified 13 x: csrc/wall_forces.hip)
 *   2 r_cut   3 r_extrap   4 shift energy (V(r_cut) or 0)   5 V(e)   6 F_e   7 Colloid: radius a (LJ93: 0)
 * A type that feels nothing (LJ93: epsilon == 0 or r_cut == 0; Colloid: A == 0, a <= 0 or r_cut == 0) has a row of
 * zeros. The *_params_make functions return AZP_ERROR_INVALID_ARGUMENT for r_cut < 0, r_extrap < 0,
 * 0 < r_cut <= r_extrap, an unknown shift mode (XPLOR included) and, for an active Colloid type, r_cut <= a or
 * 0 < r_extrap <= a. */
#define AZP_WALL_MAX 16
#define AZP_WALL_PARAM_DOUBLES 8

typedef enum azp_wall_kind
    {
    AZP_WALL_PLANE = 0,
    AZP_WALL_SPHERE = 1,
    AZP_WALL_CYLINDER = 2
    } azp_wall_kind;

typedef struct azp_wall
    {
    uint32_t kind;    /* azp_wall_kind */
    uint32_t inside;  /* sphere, cylinder: 1 = the active side is inside; ignored for a plane */
    double origin[3];
    double axis[3];   /* plane: unit normal; cylinder: unit axis; sphere: ignored */
    double radius;    /* sphere, cylinder */
    } azp_wall;

typedef struct azp_wall_args
    {
    double* d_force;        /* N x 4, overwritten */
    double* d_virial;       /* 6 x virial_pitch, zeroed if not NULL */
    uint64_t virial_pitch;
    uint32_t N;
    uint32_t ntypes;
    const double* d_pos;    /* N x 4 */
    azp_box box;
    const double* d_params; /* ntypes x AZP_WALL_PARAM_DOUBLES */
    uint32_t n_walls;       /* 1 .. AZP_WALL_MAX */
    uint32_t block_size;    /* 0: 256 */
    azp_wall walls[AZP_WALL_MAX]; /* by value: the kernel reads them from its arguments */
    } azp_wall_args;

int azp_wall_lj93_params_make(double epsilon, double sigma, double r_cut, double r_extrap, int shift_mode, double* row);
int azp_wall_colloid_params_make(double A, double sigma, double a, double r_cut, double r_extrap, int shift_mode, double* row);
int azp_wall_forces_lj93(const azp_wall_args* args, void* stream);
int azp_wall_forces_colloid(const azp_wall_args* args, void* stream);
/* Net force the particles exert on each wall and the wall's energy: d_out[4 w .. 4 w + 3] = (-sum_i F_i^(w),
 * sum_i E_i^(w)) over rows [0, N). d_force and d_virial are not used. No atomics, every order is fixed by N: two
 * calls on the same state give the same bits. d_scratch: azp_wall_net_forces_scratch_size bytes (depends on N
 * and n_walls); too small a scratch is AZP_ERROR_INVALID_ARGUMENT. */
int azp_wall_net_forces_scratch_size(const azp_wall_args* args, uint64_t* bytes);
int azp_wall_net_forces_lj93(const azp_wall_args* args, double* d_out, void* d_scratch, uint64_t scratch_bytes, void* stream);
int azp_wall_net_forces_colloid(const azp_wall_args* args, double* d_out, void* d_scratch, uint64_t scratch_bytes, void* stream);

/* ---- displacements between two times (compute.MeanSquaredDisplacement, compute.SelfIntermediateScattering) ----
 * Not part of the reference; the semantics are DEFINED HERE. Single-domain states in a 3-D box (tilts
 * included) that does not change between the two times.
 * TIME ORIGIN. azp_displacement_origin copies the wrapped position (all four words of the row) and the image of every
 * row i < N into slot `slot` of an origin store, INDEXED BY TAG: d_origin_pos[(slot N + tag_i) 4 ..], d_origin_image[(slot
 * N + tag_i) 3 ..]. The store holds n_slots origins: n_slots x N x 4 doubles and n_slots x N x 3 int32. The tags of a
 * single-domain state are a permutation of 0 .. N-1; a row with a tag >= N is not copied (the kernels below report
 * it). build_rtag != 0: d_rtag is first filled with 0xFFFFFFFF and then d_rtag[tag_i] = i (the reverse-tag table the
 * kernels below gather through; it has to be rebuilt whenever the rows are re-indexed). d_origin_pos == NULL with
 * build_rtag != 0 builds the table alone.
 * DISPLACEMENT of the particle with tag g, row i = d_rtag[g], with plain IEEE operations in exactly this order (no
 * contraction into FMAs), h_xy = xy Ly, h_xz = xz Lz, h_yz = yz Lz rounded once on the host:
 *   dn = n_i - n0_g                                   (int32, subtracted as integers first: a particle that crossed
 *                                                      the box a thousand times loses nothing to cancellation)
 *   dx = (x_i - x0_g) + ((Lx dn_x + h_xy dn_y) + h_xz dn_z)
 *   dy = (y_i - y0_g) + (Ly dn_y + h_yz dn_z)
 *   dz = (z_i - z0_g) + Lz dn_z
 * A particle belongs to the group by its CURRENT type (the type bits of pos_i.w against d_type_mask, NULL = all).
 * A tag slot g is BAD when d_rtag[g] >= N or d_tag[d_rtag[g]] != g (a forged or duplicated tag, a stale table): it
 * adds 1 to the bad_tags word and nothing else.
 * azp_displacement_moments OVERWRITES, for every origin slot s < n_origins, one row of 14 + num_bins 8-byte words at
 * d_out + s (14 + num_bins):
 *   doubles  0 N_g | 1-3 S_x S_y S_z (sums of dx, dy, dz) | 4-9 S_xx S_yy S_zz S_xy S_xz S_yz (dx dx, ... one product
 *            each) | 10 S_4 = sum r2 r2 with r2 = (dx dx + dy dy) + dz dz | 11 zero
 *   uint64   12 bad_tags | 13 outside | 14 .. counts[num_bins]: the self part of the van Hove function. With
 *            r = sqrt(r2): r >= r_max counts in `outside`, else bin min(int(r (num_bins / r_max)), num_bins - 1), the
 *            scale num_bins / r_max rounded once on the host. num_bins == 0: no histogram work, outside stays 0.
 * A slot whose bit in active_mask (bit s) is clear has not been filled: its row is all zeros.
 * d_displacements (may be NULL): N x 3 doubles by tag, (dx, dy, dz) of EVERY particle (in the group or not) against
 * origin slot 0; zeros for a bad slot. Written only when bit 0 of active_mask is set.
 * ORDER OF SUMMATION: in TAG order, the reproducible sum of csrc/azp_reduce.hpp with (per_lane, n_blocks) =
 * reduce_shape(N): thread t of workgroup b takes the tags b 256 per_lane + j 256 + t, j < per_lane, reads the origin
 * coalesced and gathers the current row through d_rtag. A particle outside the group adds nothing. No floating-point
 * atomics: the result does not depend on the order of the rows (a sort changes no bit), two calls agree bit for bit,
 * and tests/reduction_ref.tree_sum over the per-particle terms in tag order reproduces it. Every term goes straight
 * into its lane's accumulator: ADDITION DEPTH per_lane + 6 + 3 + ceil(n_blocks / 64) + 6 (72 up to N = 2^24). The
 * integer words are counted in LDS per workgroup (uint32) and added with 64-bit integer atomics. The origins are a grid
 * dimension: workgroup (b, s) reads the current rows of its tags again for every slot.
 * d_scratch: azp_displacement_moments_scratch_size bytes = n_origins x 12 x n_blocks doubles.
 * azp_self_scattering: for n_vectors integer triples m (compute.structure_factor_vectors) and every origin slot,
 *   rho_s(m) = sum over the group of exp(-2 pi i m . (f_i - f0_g)),
 * f = fractional() of csrc/cell_bin.hpp of the WRAPPED positions at the two times. On the reciprocal lattice
 * q(m) . H dn = 2 pi m . dn is a multiple of 2 pi, so the images drop out exactly and are not read. df = f - f0 is one
 * subtraction per axis, t = h df_x + k df_y + l df_z (FMA-contracted, left to right), the term (c, -s) of
 * sincospi(2 t). One lane per vector, 256 tags per stage staged through LDS in tag order, shape, fold and depth those
 * of azp_structure_factor_amplitudes' direct path: D = 256 + stages + ceil(n_chunks / 64) + 6. Row per slot, 2 n + 2
 * doubles at d_out + s (2 n + 2): Re[n], Im[n], N_g, bad_tags; zeros for a slot that is not active. Error of a component:
 * N_g 2^-52 (c |m|_1 + 4 + D) with c = pi (2 e_f + 4) (tests/displacement_ref.py). The box has to be periodic on all
 * three axes. d_scratch: azp_self_scattering_scratch_size bytes = n_origins (2 n + 2) n_chunks doubles.
 * All three calls are asynchronous on `stream`: no host synchronisation, no readback.
 * AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written: NULL args or a NULL array the call reads or
 * writes (with N > 0); n_origins outside [1, 64]; slot >= n_slots; num_bins > AZP_RDF_MAX_BINS; num_bins > 0 with
 * r_max not positive and finite; n_vectors outside [1, AZP_SF_MAX_VECTORS]; a mask with ntypes == 0; a box length that
 * is not positive and finite (for azp_self_scattering: a non-periodic axis); too small a scratch. N == 0: the rows
 * are zeroed. */
#define AZP_DISPLACEMENT_MAX_ORIGINS 64
#define AZP_DISPLACEMENT_NSUMS 12

typedef struct azp_displacement_origin_args
    {
    const double* d_pos;       /* N x 4 at least */
    const int32_t* d_image;    /* N x 3 at least */
    const uint32_t* d_tag;     /* N at least */
    uint32_t N;
    uint32_t slot;             /* < n_slots */
    uint32_t n_slots;          /* origins the store holds */
    uint32_t build_rtag;
    double* d_origin_pos;      /* n_slots x N x 4, by tag; NULL: the reverse-tag table alone */
    int32_t* d_origin_image;   /* n_slots x N x 3, by tag */
    uint32_t* d_rtag;          /* N; written when build_rtag != 0 */
    } azp_displacement_origin_args;

typedef struct azp_displacement_args
    {
    const double* d_pos;            /* N x 4 at least (x, y, z, type bits) */
    const int32_t* d_image;         /* N x 3 at least (azp_self_scattering: not read) */
    const uint32_t* d_tag;          /* N at least */
    const uint32_t* d_rtag;         /* N: row of every tag */
    uint32_t N;
    uint32_t ntypes;
    azp_box box;
    const uint8_t* d_type_mask;     /* ntypes bytes, may be NULL */
    const double* d_origin_pos;     /* n_origins x N x 4 at least, by tag */
    const int32_t* d_origin_image;  /* n_origins x N x 3 at least, by tag (azp_self_scattering: not read) */
    uint32_t n_origins;             /* 1 .. 64: rows written */
    uint32_t num_bins;              /* moments: 0 .. AZP_RDF_MAX_BINS */
    uint64_t active_mask;           /* bit s: slot s holds an origin */
    double r_max;                   /* moments, with num_bins > 0 */
    double* d_displacements;        /* moments: N x 3 by tag against slot 0, may be NULL */
    uint32_t n_vectors;             /* scattering: 1 .. AZP_SF_MAX_VECTORS */
    uint32_t _pad;
    const int32_t* d_vectors;       /* scattering: n_vectors x 3 */
    void* d_out;                    /* n_origins rows, overwritten */
    void* d_scratch;
    uint64_t scratch_bytes;
    } azp_displacement_args;

int azp_displacement_origin(const azp_displacement_origin_args* args, void* stream);
int azp_displacement_moments_scratch_size(const azp_displacement_args* args, uint64_t* bytes);
int azp_displacement_moments(const azp_displacement_args* args, void* stream);
int azp_self_scattering_scratch_size(const azp_displacement_args* args, uint64_t* bytes);
int azp_self_scattering(const azp_displacement_args* args, void* stream);

/* ---- pressure profile (compute.PressureProfile) ----
 * Not part of the reference; the semantics are DEFINED HERE. The configurational part of the
 * Irving-Kirkwood contour stress along one Cartesian axis (0, 1, 2 = x, y, z), in num_bins equal bins on
 * [lower, lower + num_bins / scale): scale = num_bins / (upper - lower) is computed once by the caller and passed in.
 *
 * A pair. Every unordered pair (i, j) that the force acts on is taken ONCE, with i the member with the smaller tag:
 *   d = minimum image of r_i - r_j (the image code of the force kernels), rsq = d.x d.x + d.y d.y + d.z d.z as
 *   walk_accept writes it; force_divr from the force's evaluator (E::prepare / E::eval with the force's r_cut^2 and
 *   r_on^2 tables and shift_mode, xplor through apply_xplor, exactly as the pair kernels call them); a pair that the
 *   evaluator does not evaluate (beyond its r_cut, a bond that its evaluator rejects) contributes nothing and is not
 *   counted. The six virial words are w = {fx d.x, fx d.y, fx d.z, fy d.y, fy d.z, fz d.z} with fx = force_divr d.x,
 *   fy = force_divr d.y, fz = force_divr d.z.
 * The weights. With z1 = the stored coordinate of i along the axis and da = d[axis], every operation rounded once (no
 * contraction):
 *   s1 = (z1 - lower) * scale;  s0 = ((z1 - da) - lower) * scale;  lo = min(s0, s1);  hi = max(s0, s1);
 *   if floor(lo) == floor(hi): the one bin k = floor(lo) gets lambda = 1 (da = 0 is this case);
 *   else for every integer k from floor(lo) to floor(hi): lambda_k = (min(hi, k + 1) - max(lo, k)) / (hi - lo), and a
 *   bin with lambda_k <= 0 (an end point exactly on an edge) gets nothing.
 *   wrap != 0 (the range is the whole box length of a periodic axis): k is taken modulo num_bins; wrap == 0: a k
 *   outside [0, num_bins) is dropped. |lo| or |hi| >= 1e9 or not finite: the pair's six words count as overflow.
 * A term is t = lambda_k * w[c]. If t is not finite or |t| >= max_term it is NOT added and the overflow word counts it;
 * else q = round-to-nearest-even(t * 2^shift) is added to word 6 k + c of the row with a 64-bit integer atomic (in
 * LDS first where num_bins <= AZP_PRESSURE_PROFILE_LDS_BINS, else straight into the row). Integers only: a row is the
 * same bits between two calls, between the paths, and under a reordering of the rows that carries the tags.
 *
 * The row at d_out is 6 num_bins + 4 int64 words: the bins (xx, xy, xz, yy, yz, zz each), then pairs evaluated, terms
 * added, terms refused (overflow), shift. azp_pressure_profile_begin zeroes it on the stream and writes the shift;
 * every other call ADDS to it, so the forces of an integrator are summed by calling one after the other:
 *   azp_pressure_profile_pairs_<potential>  all pairs closer than r_max (the largest r_cut of the force), by the walk
 *       of azp_rdf_counts: path 0 = automatic, 1 = all-pairs (any box), 2 = cells (orthorhombic, at least three cells
 *       of width r_max on every periodic axis; refused elsewhere, never silently replaced). d_scratch:
 *       azp_pressure_profile_scratch_size bytes (0 for all-pairs). r_max beyond half a perpendicular width of a
 *       periodic axis is refused. Table and the conservative DPD force take shift_mode AZP_SHIFT_NONE only.
 *   azp_pressure_profile_listed  the pairs of a per-particle table (entry s of row i at s * pitch + i, s < d_counts[i]),
 *       each taken from the row with the smaller tag, multiplied by sign (+1 / -1; a pass with -1 also counts the
 *       summary words down). A pair evaluator (AZP_PP_PERTURBED_LENNARD_JONES .. AZP_PP_PAIR_TABLE): d_table holds
 *       uint32 partner rows, the symmetric exclusion table of a neighbor list; with sign -1 behind the walk it takes
 *       out exactly what the walk added, because a pair's terms are a function of the pair alone. A bond evaluator
 *       (AZP_PP_BOND_DOUBLE_WELL .. AZP_PP_SPECIAL_PAIR_LJ): d_table holds azp_bond_entry (the bond table, which the
 *       special pairs share), d_params n_types parameter structs; d_rcutsq, d_ronsq, r_max are not read.
 *   An entry that names a row >= N, the row itself or a type >= n_types is skipped.
 * Single-domain states only (N rows, no ghosts). AZP_ERROR_INVALID_ARGUMENT, before anything is launched or written:
 * NULL args or a NULL array the call reads; axis > 2; num_bins < 1 or > AZP_PRESSURE_PROFILE_MAX_BINS; scale or max_term
 * not positive and finite; shift > 52; ntypes == 0; and per call what is said above. AZP_ERROR_TOO_MANY_TYPES: the
 * coefficient table does not fit beside the histogram. N == 0: success. Asynchronous on `stream`. */
#define AZP_PRESSURE_PROFILE_MAX_BINS 8192
#define AZP_PRESSURE_PROFILE_LDS_BINS 1024

typedef enum azp_pressure_profile_evaluator
    {
    AZP_PP_PERTURBED_LENNARD_JONES = 0,
    AZP_PP_HERTZ = 1,
    AZP_PP_EXPANDED_YUKAWA = 2,
    AZP_PP_COLLOID = 3,
    AZP_PP_DPD_CONSERVATIVE = 4,
    AZP_PP_PAIR_TABLE = 5,
    AZP_PP_BOND_DOUBLE_WELL = 16,
    AZP_PP_BOND_QUARTIC = 17,
    AZP_PP_BOND_TABLE = 18,
    AZP_PP_SPECIAL_PAIR_LJ = 19
    } azp_pressure_profile_evaluator;

typedef struct azp_pressure_profile_args
    {
    const double* d_pos;      /* N x 4 (x, y, z, type bits) */
    const uint32_t* d_tag;    /* N */
    uint32_t N;
    uint32_t ntypes;
    azp_box box;
    uint32_t axis;            /* 0, 1, 2 */
    uint32_t num_bins;
    double lower;
    double scale;             /* num_bins / (upper - lower) */
    double max_term;
    uint32_t wrap;            /* bin indices modulo num_bins */
    uint32_t shift;           /* terms in units of 2^-shift */
    const double* d_rcutsq;   /* ntypes x ntypes (pair evaluators) */
    const double* d_ronsq;    /* ntypes x ntypes (AZP_SHIFT_XPLOR) */
    double r_max;             /* the radius of the walk: the largest r_cut */
    uint32_t shift_mode;      /* azp_shift_mode */
    uint32_t path;            /* 0 auto, 1 all-pairs, 2 cells */
    int64_t* d_out;           /* 6 num_bins + 4 */
    void* d_scratch;
    uint64_t scratch_bytes;
    } azp_pressure_profile_args;

typedef struct azp_pressure_profile_list_args
    {
    azp_pressure_profile_args profile; /* path, d_scratch and scratch_bytes are not looked at */
    const void* d_table;
    const uint32_t* d_counts;          /* N */
    uint64_t pitch;
    uint32_t n_types;                  /* bond evaluators: parameter structs at d_params */
    uint32_t evaluator;                /* azp_pressure_profile_evaluator */
    int32_t sign;                      /* +1 or -1 */
    uint32_t _pad;
    } azp_pressure_profile_list_args;

int azp_pressure_profile_scratch_size(const azp_pressure_profile_args* args, uint64_t* bytes);
int azp_pressure_profile_begin(const azp_pressure_profile_args* args, void* stream);
int azp_pressure_profile_pairs_perturbed_lennard_jones(const azp_pressure_profile_args* args, const azp_plj_params* d_params, void* stream);
int azp_pressure_profile_pairs_hertz(const azp_pressure_profile_args* args, const azp_hertz_params* d_params, void* stream);
int azp_pressure_profile_pairs_expanded_yukawa(const azp_pressure_profile_args* args, const azp_yukawa_params* d_params, void* stream);
int azp_pressure_profile_pairs_colloid(const azp_pressure_profile_args* args, const azp_colloid_params* d_params, void* stream);
int azp_pressure_profile_pairs_dpd_conservative(const azp_pressure_profile_args* args, const azp_dpd_params* d_params, void* stream);
int azp_pressure_profile_pairs_table(const azp_pressure_profile_args* args, const azp_table_params* d_params, void* stream);
int azp_pressure_profile_listed(const azp_pressure_profile_list_args* args, const void* d_params, void* stream);

/* ---- misc ---- */
int azp_version(void);                  /* major * 1000 + minor       */
const char* azp_status_string(int status);
/* Resolved launch configuration of the last pair-force call on this thread
 * (for benchmarks / profiling reports). */
void azp_last_launch(uint32_t* block_size, uint32_t* threads_per_particle, uint32_t* grid, uint32_t* lds_bytes);
/* The library has no process-wide switches. Two exact options of the tile kernel were measured and removed (last
 * present in 26438a0): test-free / core-test-free row phases (1.5 % slower on the north star although
 * they issue fewer instructions) and two launches by staged-set size (5 % slower). azp_pair_args.d_displacement is used
 * whenever it is given together with a valid displacement bound. */

#ifdef __cplusplus
}
#endif
#endif /* AZP_H_ */
