"""ctypes binding of ``libazp.so`` (the C ABI declared in ``include/azp.h``).

The product path has no CPU fallback: if the HIP library is missing or a call
fails, an exception is raised.
"""

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AZP_LIB_PATH", os.path.join(_HERE, "libazp.so"))  # env override: kernel experiments only
CSRC = os.path.join(_HERE, "csrc")


class AzpError(RuntimeError):
    pass


# ---------------------------------------------------------------------------
# structs (field order = include/azp.h)
# ---------------------------------------------------------------------------
class Box(C.Structure):
    _fields_ = [("L", C.c_double * 3), ("tilt", C.c_double * 3), ("periodic", C.c_int32 * 3), ("_pad", C.c_int32)]


class PairArgs(C.Structure):
    _fields_ = [
        ("d_force", C.c_void_p),
        ("d_virial", C.c_void_p),
        ("virial_pitch", C.c_uint64),
        ("N", C.c_uint32),
        ("n_max", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("d_n_neigh", C.c_void_p),
        ("d_nlist", C.c_void_p),
        ("d_head_list", C.c_void_p),
        ("d_rcutsq", C.c_void_p),
        ("d_ronsq", C.c_void_p),
        ("size_nlist", C.c_uint64),
        ("ntypes", C.c_uint32),
        ("shift_mode", C.c_uint32),
        ("compute_virial", C.c_uint32),
        ("block_size", C.c_uint32),
        ("threads_per_particle", C.c_uint32),
        ("flags", C.c_uint32),
        ("range_first", C.c_uint32),
        ("range_count", C.c_uint32),
        ("r_list_max", C.c_double),
        ("d_rinnersq", C.c_void_p),
        ("has_displacement_bound", C.c_uint32),
        ("_pad3", C.c_uint32),
        ("displacement_bound", C.c_double),
        ("d_displacement", C.c_void_p),
        ("list_generation", C.c_uint64),
        ("d_stale_flag", C.c_void_p),
        ("d_displacement_sq_bits", C.c_void_p),
        ("displacement_bound_extra", C.c_double),
    ]


class TableParams(C.Structure):
    _fields_ = [("r_min", C.c_double), ("r_max", C.c_double), ("d_rows", C.c_void_p), ("n", C.c_uint32), ("_pad", C.c_uint32)]


class DPDArgs(C.Structure):
    _fields_ = [
        ("pair", PairArgs),
        ("d_vel", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("timestep", C.c_uint64),
        ("deltaT", C.c_double),
        ("T", C.c_double),
        ("seed", C.c_uint16),
        ("_pad", C.c_uint16 * 3),
    ]


class AnisoArgs(C.Structure):
    _fields_ = [("pair", PairArgs), ("d_orientation", C.c_void_p), ("d_torque", C.c_void_p)]


class BondArgs(C.Structure):
    _fields_ = [
        ("d_force", C.c_void_p),
        ("d_virial", C.c_void_p),
        ("virial_pitch", C.c_uint64),
        ("N", C.c_uint32),
        ("n_max", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("d_gpu_bondlist", C.c_void_p),
        ("d_gpu_bond_pos", C.c_void_p),
        ("d_gpu_n_bonds", C.c_void_p),
        ("pitch", C.c_uint64),
        ("n_bond_types", C.c_uint32),
        ("compute_virial", C.c_uint32),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class PairGroupArgs(C.Structure):
    """azp_special_pair_args (``BondedForce`` finds a kind's struct as ``<Kind>Args``: the special pairs are the kind
    "pair"; ``PairArgs`` is the non-bonded pair kernels')."""

    _fields_ = [
        ("d_force", C.c_void_p),
        ("d_virial", C.c_void_p),
        ("virial_pitch", C.c_uint64),
        ("N", C.c_uint32),
        ("n_max", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("d_gpu_pairlist", C.c_void_p),
        ("d_gpu_pair_pos", C.c_void_p),
        ("d_gpu_n_pairs", C.c_void_p),
        ("pitch", C.c_uint64),
        ("n_pair_types", C.c_uint32),
        ("compute_virial", C.c_uint32),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class AngleEntry(C.Structure):
    _fields_ = [("idx", C.c_uint32 * 2), ("type", C.c_uint32), ("pos", C.c_uint32)]


class AngleArgs(C.Structure):
    _fields_ = [
        ("d_force", C.c_void_p),
        ("d_virial", C.c_void_p),
        ("virial_pitch", C.c_uint64),
        ("N", C.c_uint32),
        ("n_max", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("d_gpu_anglelist", C.c_void_p),
        ("d_gpu_n_angles", C.c_void_p),
        ("pitch", C.c_uint64),
        ("n_angle_types", C.c_uint32),
        ("compute_virial", C.c_uint32),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class DihedralEntry(C.Structure):
    _fields_ = [("idx", C.c_uint32 * 3), ("type_pos", C.c_uint32)]


class DihedralPeriodicParams(C.Structure):
    _fields_ = [("k", C.c_double), ("cos_phi0", C.c_double), ("sin_phi0", C.c_double), ("d", C.c_int32), ("n", C.c_uint32)]


class DihedralArgs(C.Structure):
    _fields_ = [
        ("d_force", C.c_void_p),
        ("d_virial", C.c_void_p),
        ("virial_pitch", C.c_uint64),
        ("N", C.c_uint32),
        ("n_max", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("d_gpu_dihedrallist", C.c_void_p),
        ("d_gpu_n_dihedrals", C.c_void_p),
        ("pitch", C.c_uint64),
        ("n_dihedral_types", C.c_uint32),
        ("compute_virial", C.c_uint32),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class BarrierArgs(C.Structure):
    _fields_ = [
        ("d_force", C.c_void_p),
        ("d_virial", C.c_void_p),
        ("virial_pitch", C.c_uint64),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("d_params", C.c_void_p),
        ("location", C.c_double),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class NVEArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("d_net_force", C.c_void_p),
        ("d_image", C.c_void_p),
        ("box", Box),
        ("dt", C.c_double),
        ("N", C.c_uint32),
        ("block_size", C.c_uint32),
    ]


class NVERotArgs(C.Structure):
    _fields_ = [
        ("d_orientation", C.c_void_p),
        ("d_angmom", C.c_void_p),
        ("d_inertia", C.c_void_p),
        ("d_net_torque", C.c_void_p),
        ("dt", C.c_double),
        ("N", C.c_uint32),
        ("block_size", C.c_uint32),
    ]


class PlanInfo(C.Structure):
    _fields_ = [
        ("valid", C.c_int32),
        ("invalid_reason", C.c_int32),
        ("threads_per_particle", C.c_uint32),
        ("tile_size", C.c_uint32),
        ("lds_slots", C.c_uint32),
        ("n_tiles", C.c_uint32),
        ("max_stage", C.c_uint32),
        ("max_row", C.c_uint32),
        ("total_stage", C.c_uint64),
        ("compiled_bytes", C.c_uint64),
        ("builds", C.c_uint64),
        ("from_cells", C.c_int32),
        ("row_capacity", C.c_uint32),
        ("list_id", C.c_uint64),
        ("head_id", C.c_uint64),
        ("balanced", C.c_int32),
        ("core_radius", C.c_float),
        ("sure_radius", C.c_float),
        ("max_member_cells", C.c_uint32),
    ]


class AutoPlanStats(C.Structure):
    _fields_ = [("calls", C.c_uint64), ("compiles", C.c_uint64), ("reuses", C.c_uint64), ("generic_fallbacks", C.c_uint64)]


PAIR_FLAG_NO_AUTO_PLAN = 1
ERROR_TOO_MANY_TYPES = -2


class HaloField(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("row_bytes", C.c_uint32), ("_pad", C.c_uint32)]


class CellGrid(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("width", C.c_double * 3), ("dim", C.c_uint32 * 3), ("periodic", C.c_int32 * 3)]


class NlistArgs(C.Structure):
    _fields_ = [
        ("N", C.c_uint32),
        ("n_total", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("grid", CellGrid),
        ("ntypes", C.c_uint32),
        ("cell_subdivision", C.c_uint32),
        ("d_rlistsq", C.c_void_p),
        ("d_cell_of", C.c_void_p),
        ("d_cell_sorted", C.c_void_p),
        ("d_order", C.c_void_p),
        ("d_cell_start", C.c_void_p),
        ("d_n_excl", C.c_void_p),
        ("d_excl", C.c_void_p),
        ("excl_pitch", C.c_uint64),
        ("d_n_neigh", C.c_void_p),
        ("d_head_list", C.c_void_p),
        ("d_nlist", C.c_void_p),
        ("row_capacity", C.c_uint32),
        ("fractional_cells", C.c_uint32),
        ("d_max_neigh", C.c_void_p),
    ]


COORDINATES_CARTESIAN = 0
COORDINATES_CYLINDRICAL = 1
MAX_BINS = 2**31 - 1


class VelocityFieldArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("N", C.c_uint32),
        ("coordinates", C.c_uint32),
        ("box", Box),
        ("num_bins", C.c_uint32 * 3),
        ("ntypes", C.c_uint32),
        ("lower", C.c_double * 3),
        ("upper", C.c_double * 3),
        ("d_type_mask", C.c_void_p),
        ("d_sums", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
    ]


THERMO_NSUMS = 20
THERMO_MAX_FORCES = 8


class ThermoArgs(C.Structure):
    _fields_ = [
        ("d_vel", C.c_void_p),
        ("d_pos", C.c_void_p),
        ("d_type_mask", C.c_void_p),
        ("d_force", C.c_void_p * THERMO_MAX_FORCES),
        ("d_virial", C.c_void_p * THERMO_MAX_FORCES),
        ("d_orientation", C.c_void_p),
        ("d_angmom", C.c_void_p),
        ("d_inertia", C.c_void_p),
        ("d_out", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("n_forces", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


THERMO_FIELD_NSUMS = 18
THERMO_FIELD_NO_BIN = 0x7FFFFFFF
THERMO_FIELD_HEADS, THERMO_FIELD_LEVELS = 1, 2  # ThermoFieldArgs.phases, for timing alone (0: everything)


class ThermoFieldArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("d_type_mask", C.c_void_p),
        ("d_force", C.c_void_p * THERMO_MAX_FORCES),
        ("d_virial", C.c_void_p * THERMO_MAX_FORCES),
        ("d_keys", C.c_void_p),
        ("d_sorted_keys", C.c_void_p),
        ("d_order", C.c_void_p),
        ("d_out", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
        ("box", Box),
        ("lower", C.c_double * 3),
        ("upper", C.c_double * 3),
        ("num_bins", C.c_uint32 * 3),
        ("coordinates", C.c_uint32),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("n_forces", C.c_uint32),
        ("phases", C.c_uint32),
    ]


RDF_MAX_BINS = 8192
RDF_PATH_AUTO, RDF_PATH_ALL_PAIRS, RDF_PATH_CELLS = 0, 1, 2


class RdfArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("N", C.c_uint32),
        ("n_total", C.c_uint32),
        ("box", Box),
        ("ntypes", C.c_uint32),
        ("num_bins", C.c_uint32),
        ("d_type_mask_a", C.c_void_p),
        ("d_type_mask_b", C.c_void_p),
        ("r_max", C.c_double),
        ("scale", C.c_double),
        ("path", C.c_uint32),
        ("_pad", C.c_uint32),
        ("d_out", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
    ]


class RdfExclusionArgs(C.Structure):
    _fields_ = [("rdf", RdfArgs), ("d_n_excl", C.c_void_p), ("d_excl", C.c_void_p), ("excl_pitch", C.c_uint64)]


PRESSURE_PROFILE_MAX_BINS = 8192
PRESSURE_PROFILE_LDS_BINS = 1024
# azp_pressure_profile_evaluator
PP_EVALUATORS = dict(PerturbedLennardJones=0, Hertz=1, ExpandedYukawa=2, Colloid=3, DPDConservativeGeneralWeight=4, PairTable=5,
                     DoubleWell=16, Quartic=17, BondTable=18, SpecialPairLJ=19)


class PressureProfileArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("box", Box),
        ("axis", C.c_uint32),
        ("num_bins", C.c_uint32),
        ("lower", C.c_double),
        ("scale", C.c_double),
        ("max_term", C.c_double),
        ("wrap", C.c_uint32),
        ("shift", C.c_uint32),
        ("d_rcutsq", C.c_void_p),
        ("d_ronsq", C.c_void_p),
        ("r_max", C.c_double),
        ("shift_mode", C.c_uint32),
        ("path", C.c_uint32),
        ("d_out", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
    ]


class PressureProfileListArgs(C.Structure):
    _fields_ = [
        ("profile", PressureProfileArgs),
        ("d_table", C.c_void_p),
        ("d_counts", C.c_void_p),
        ("pitch", C.c_uint64),
        ("n_types", C.c_uint32),
        ("evaluator", C.c_uint32),
        ("sign", C.c_int32),
        ("_pad", C.c_uint32),
    ]


STEINHARDT_MAX_TERMS = 4
STEINHARDT_MAX_L = 12
STEINHARDT_MAX_BINS = 1024
STEINHARDT_MAX_N = 1 << 21
STEINHARDT_AVERAGE, STEINHARDT_CONNECTIONS = 1, 2
STEINHARDT_CONNECTION_BINS = 33
STEINHARDT_PATH_AUTO, STEINHARDT_PATH_ALL_PAIRS, STEINHARDT_PATH_CELLS = 0, 1, 2


class SteinhardtArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("box", Box),
        ("d_type_mask", C.c_void_p),
        ("r_max", C.c_double),
        ("q_threshold", C.c_double),
        ("solid_threshold", C.c_uint32),
        ("n_terms", C.c_uint32),
        ("l", C.c_uint32 * STEINHARDT_MAX_TERMS),
        ("norm", (C.c_double * (STEINHARDT_MAX_L + 1)) * STEINHARDT_MAX_TERMS),
        ("flags", C.c_uint32),
        ("path", C.c_uint32),
        ("num_bins", C.c_uint32),
        ("_pad", C.c_uint32),
        ("d_num_neighbors", C.c_void_p),
        ("d_words", C.c_void_p),
        ("d_order", C.c_void_p),
        ("d_avg_words", C.c_void_p),
        ("d_num_connections", C.c_void_p),
        ("d_summary", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
    ]


CLUSTER_NONE = 0xFFFFFFFF
CLUSTER_MAX_BINS = 1024
CLUSTER_MAX_N = 1 << 30
CLUSTER_PATH_AUTO, CLUSTER_PATH_ALL_PAIRS, CLUSTER_PATH_CELLS = 0, 1, 2


class ClusterArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("box", Box),
        ("d_type_mask", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("d_member", C.c_void_p),
        ("member_min", C.c_uint32),
        ("path", C.c_uint32),
        ("r_max", C.c_double),
        ("size_bins", C.c_uint32),
        ("stages", C.c_uint32),
        ("d_cluster_key", C.c_void_p),
        ("d_cluster_size", C.c_void_p),
        ("d_summary", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
        ("d_cluster_rep", C.c_void_p),
    ]


CLUSTER_PROPERTIES_ROW = 16
CLUSTER_PROPERTIES_SUMMARY = 20


class ClusterPropertiesArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("N", C.c_uint32),
        ("min_size", C.c_uint32),
        ("box", Box),
        ("d_cluster_rep", C.c_void_p),
        ("d_cluster_key", C.c_void_p),
        ("d_cluster_size", C.c_void_p),
        ("d_table", C.c_void_p),
        ("d_summary", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
    ]


BONDED_HISTOGRAM_LDS_WORDS = 16384
BONDED_HISTOGRAM_PATH_AUTO, BONDED_HISTOGRAM_PATH_LDS, BONDED_HISTOGRAM_PATH_GLOBAL = 0, 1, 2


class BondedHistogramArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("N", C.c_uint32),
        ("n_max", C.c_uint32),
        ("box", Box),
        ("arity", C.c_uint32),
        ("n_types", C.c_uint32),
        ("d_table", C.c_void_p),
        ("d_table_pos", C.c_void_p),
        ("d_counts", C.c_void_p),
        ("pitch", C.c_uint64),
        ("num_bins", C.c_uint32),
        ("path", C.c_uint32),
        ("r_min", C.c_double),
        ("r_max", C.c_double),
        ("d_out", C.c_void_p),
    ]


SF_MAX_VECTORS = 65536
SF_POWERS_LDS_BYTES = 49152
SF_PATH_AUTO, SF_PATH_DIRECT, SF_PATH_POWERS = 0, 1, 2


class StructureFactorArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("box", Box),
        ("d_type_mask_a", C.c_void_p),
        ("d_type_mask_b", C.c_void_p),
        ("same_groups", C.c_uint32),
        ("n_vectors", C.c_uint32),
        ("d_vectors", C.c_void_p),
        ("m_max", C.c_uint32 * 3),
        ("path", C.c_uint32),
        ("d_out", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
    ]


DISPLACEMENT_MAX_ORIGINS = 64
DISPLACEMENT_NSUMS = 12


class DisplacementOriginArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("N", C.c_uint32),
        ("slot", C.c_uint32),
        ("n_slots", C.c_uint32),
        ("build_rtag", C.c_uint32),
        ("d_origin_pos", C.c_void_p),
        ("d_origin_image", C.c_void_p),
        ("d_rtag", C.c_void_p),
    ]


class DisplacementArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("d_rtag", C.c_void_p),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("box", Box),
        ("d_type_mask", C.c_void_p),
        ("d_origin_pos", C.c_void_p),
        ("d_origin_image", C.c_void_p),
        ("n_origins", C.c_uint32),
        ("num_bins", C.c_uint32),
        ("active_mask", C.c_uint64),
        ("r_max", C.c_double),
        ("d_displacements", C.c_void_p),
        ("n_vectors", C.c_uint32),
        ("_pad", C.c_uint32),
        ("d_vectors", C.c_void_p),
        ("d_out", C.c_void_p),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
    ]


FLOW_CONSTANT = 0
FLOW_PARABOLIC = 1


class Flow(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("_pad", C.c_uint32), ("p", C.c_double * 3)]


class FlowMethodArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("d_accel", C.c_void_p),
        ("d_net_force", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("d_gamma", C.c_void_p),
        ("d_type_mask", C.c_void_p),
        ("box", Box),
        ("dt", C.c_double),
        ("kT", C.c_double),
        ("timestep", C.c_uint64),
        ("seed", C.c_uint32),
        ("noiseless", C.c_uint32),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("flow", Flow),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class LangevinArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("d_accel", C.c_void_p),
        ("d_net_force", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("d_gamma", C.c_void_p),
        ("d_type_mask", C.c_void_p),
        ("d_orientation", C.c_void_p),
        ("d_angmom", C.c_void_p),
        ("d_inertia", C.c_void_p),
        ("d_net_torque", C.c_void_p),
        ("d_langevin_torque", C.c_void_p),
        ("d_gamma_r", C.c_void_p),
        ("box", Box),
        ("dt", C.c_double),
        ("kT", C.c_double),
        ("timestep", C.c_uint64),
        ("seed", C.c_uint32),
        ("rotational", C.c_uint32),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


THERMOSTAT_BERENDSEN, THERMOSTAT_BUSSI, THERMOSTAT_MTTK = 0, 1, 2
THERMOSTAT_NSTATE = 8
(THERMOSTAT_ALPHA, THERMOSTAT_K, THERMOSTAT_ENERGY, THERMOSTAT_XI, THERMOSTAT_ETA, THERMOSTAT_ATTEMPTS) = range(6)


class ThermostatArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("d_net_force", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_partials", C.c_void_p),
        ("d_state", C.c_void_p),
        ("partials_bytes", C.c_uint64),
        ("box", Box),
        ("dt", C.c_double),
        ("kT", C.c_double),
        ("tau", C.c_double),
        ("ndof", C.c_double),
        ("timestep", C.c_uint64),
        ("seed", C.c_uint32),
        ("kind", C.c_uint32),
        ("N", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


BAROSTAT_NSTATE = 24
(BAROSTAT_NU, BAROSTAT_ALPHA, BAROSTAT_LAMBDA, BAROSTAT_B) = (0, 3, 6, 9)  # three slots each: x, y, z
(BAROSTAT_ALPHA_T, BAROSTAT_ENERGY, BAROSTAT_V, BAROSTAT_P, BAROSTAT_NONFINITE, BAROSTAT_REF_KT, BAROSTAT_K, BAROSTAT_W) = (
    12, 13, 14, 15, 18, 19, 20, 21)
BAROSTAT_CLOSE, BAROSTAT_OPEN = 1, 2
BAROSTAT_COUPLE = {"none": 0, "xy": 1, "xz": 2, "yz": 3, "xyz": 4}


class BarostatArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("d_net_force", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_state", C.c_void_p),
        ("d_sums", C.c_void_p),
        ("d_thermostat_state", C.c_void_p),
        ("box", Box),
        ("dt", C.c_double),
        ("S", C.c_double * 3),
        ("tauS", C.c_double),
        ("ndof", C.c_double),
        ("thermostat_kT", C.c_double),
        ("thermostat_tau", C.c_double),
        ("timestep", C.c_uint64),
        ("thermostat_kind", C.c_uint32),
        ("thermostat_seed", C.c_uint32),
        ("couple", C.c_uint32),
        ("box_dof", C.c_uint32),
        ("phase", C.c_uint32),
        ("N", C.c_uint32),
    ]


FIRE_NSTATE = 16
(FIRE_DT, FIRE_ALPHA, FIRE_KEEP, FIRE_MIX, FIRE_N_POS, FIRE_N_STEPS, FIRE_U, FIRE_U_PREV, FIRE_P, FIRE_VV, FIRE_FF, FIRE_CONVERGED,
 FIRE_NONFINITE) = range(13)
FIRE_NSLOTS = 4


class FireArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_vel", C.c_void_p),
        ("d_net_force", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_partials", C.c_void_p),
        ("d_state", C.c_void_p),
        ("partials_bytes", C.c_uint64),
        ("box", Box),
        ("dt_max", C.c_double),
        ("force_tol", C.c_double),
        ("energy_tol", C.c_double),
        ("finc_dt", C.c_double),
        ("fdec_dt", C.c_double),
        ("alpha_start", C.c_double),
        ("fdec_alpha", C.c_double),
        ("min_steps_adapt", C.c_uint32),
        ("min_steps_conv", C.c_uint32),
        ("N", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class TypeUpdateArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("N", C.c_uint32),
        ("inside_type", C.c_uint32),
        ("outside_type", C.c_uint32),
        ("block_size", C.c_uint32),
        ("z_lo", C.c_double),
        ("z_hi", C.c_double),
    ]


class BoxResizeArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_image", C.c_void_p),
        ("d_type_mask", C.c_void_p),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("block_size", C.c_uint32),
        ("_pad", C.c_uint32),
        ("M", C.c_double * 6),
        ("box", Box),
    ]


EVAPORATE_NO_LIMIT = 0xFFFFFFFF


class EvaporateArgs(C.Structure):
    _fields_ = [
        ("d_pos", C.c_void_p),
        ("d_tag", C.c_void_p),
        ("N", C.c_uint32),
        ("solvent_type", C.c_uint32),
        ("evaporated_type", C.c_uint32),
        ("Nmax", C.c_uint32),
        ("z_lo", C.c_double),
        ("z_hi", C.c_double),
        ("timestep", C.c_uint64),
        ("seed", C.c_uint32),
        ("block_size", C.c_uint32),
        ("d_scratch", C.c_void_p),
        ("scratch_bytes", C.c_uint64),
        ("d_counts", C.c_void_p),
        ("d_keys_out", C.c_void_p),
        ("d_n_keys_out", C.c_void_p),
    ]


WALL_MAX = 16
WALL_PARAM_DOUBLES = 8
WALL_PLANE = 0
WALL_SPHERE = 1
WALL_CYLINDER = 2


class Wall(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("inside", C.c_uint32), ("origin", C.c_double * 3), ("axis", C.c_double * 3),
                ("radius", C.c_double)]


class WallArgs(C.Structure):
    _fields_ = [
        ("d_force", C.c_void_p),
        ("d_virial", C.c_void_p),
        ("virial_pitch", C.c_uint64),
        ("N", C.c_uint32),
        ("ntypes", C.c_uint32),
        ("d_pos", C.c_void_p),
        ("box", Box),
        ("d_params", C.c_void_p),
        ("n_walls", C.c_uint32),
        ("block_size", C.c_uint32),
        ("walls", Wall * WALL_MAX),
    ]


# every symbol include/azp.h declares: name -> (restype, argtypes)
_D = C.c_double
_PD = C.POINTER(C.c_double)
_PI = C.POINTER(C.c_int)
_VP = C.c_void_p
SYMBOLS = {
    "azp_plj_params_make": (None, [_D] * 3 + [_VP]),
    "azp_plj_params_unpack": (None, [_VP] + [_PD] * 3),
    "azp_colloid_params_make": (None, [_D] * 4 + [_VP]),
    "azp_colloid_params_unpack": (None, [_VP] + [_PD] * 4),
    "azp_tpm_params_make": (None, [_D] * 5 + [C.c_int, _VP]),
    "azp_tpm_params_unpack": (None, [_VP] + [_PD] * 5 + [_PI]),
    "azp_dw_params_make": (None, [_D] * 4 + [_VP]),
    "azp_dw_params_unpack": (None, [_VP] + [_PD] * 4),
    "azp_quartic_params_make": (None, [_D] * 8 + [_VP]),
    "azp_quartic_params_unpack": (None, [_VP] + [_PD] * 8),
    "azp_table_pack": (C.c_int, [_D, _D, _VP, _VP, C.c_uint32, C.c_int, _VP]),
    "azp_pair_forces_table": (C.c_int, [C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_planned_table": (C.c_int, [_VP, C.POINTER(PairArgs), _VP, _VP]),
    "azp_bond_forces_table": (C.c_int, [C.POINTER(BondArgs), _VP, _VP, _VP]),
    "azp_pair_forces_perturbed_lennard_jones": (C.c_int, [C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_hertz": (C.c_int, [C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_expanded_yukawa": (C.c_int, [C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_colloid": (C.c_int, [C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_dpd_conservative": (C.c_int, [C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_plan_create": (C.c_int, [C.POINTER(_VP)]),
    "azp_pair_plan_destroy": (None, [_VP]),
    "azp_pair_plan_build": (C.c_int, [_VP, C.POINTER(PairArgs), _VP]),
    "azp_pair_plan_build_from_cells": (C.c_int, [_VP, C.POINTER(NlistArgs), C.POINTER(PairArgs), _VP]),
    "azp_pair_plan_set_bank_order": (C.c_int, [_VP, C.c_int]),
    "azp_pair_plan_set_balance": (C.c_int, [_VP, C.c_int]),
    "azp_pair_plan_tile_stage": (C.c_int, [_VP, C.POINTER(C.c_uint32), C.c_uint32]),
    "azp_pair_plan_query": (C.c_int, [_VP, C.POINTER(PlanInfo)]),
    "azp_pair_plan_phase_chunks": (C.c_int, [_VP, C.POINTER(C.c_float)]),
    "azp_pair_plan_shells": (C.c_uint32, []),
    "azp_pair_plan_shells_for": (C.c_uint32, [_D, C.c_int, _D]),
    "azp_pair_plan_row_batches": (C.c_int, [_VP, C.POINTER(C.c_uint32), C.c_uint32, _PD]),
    "azp_sum_forces": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), _VP, _VP]),
    "azp_pair_auto_plan_get_stats": (None, [C.POINTER(AutoPlanStats)]),
    "azp_pair_auto_plan_clear": (None, []),
    "azp_pair_forces_planned_perturbed_lennard_jones": (C.c_int, [_VP, C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_planned_hertz": (C.c_int, [_VP, C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_planned_expanded_yukawa": (C.c_int, [_VP, C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_planned_colloid": (C.c_int, [_VP, C.POINTER(PairArgs), _VP, _VP]),
    "azp_pair_forces_planned_dpd_conservative": (C.c_int, [_VP, C.POINTER(PairArgs), _VP, _VP]),
    "azp_dpd_forces_general_weight": (C.c_int, [C.POINTER(DPDArgs), _VP, _VP]),
    "azp_aniso_forces_two_patch_morse": (C.c_int, [C.POINTER(AnisoArgs), _VP, _VP]),
    "azp_dpd_forces_planned_general_weight": (C.c_int, [_VP, C.POINTER(DPDArgs), _VP, _VP]),
    "azp_aniso_forces_planned_two_patch_morse": (C.c_int, [_VP, C.POINTER(AnisoArgs), _VP, _VP]),
    "azp_bond_forces_double_well": (C.c_int, [C.POINTER(BondArgs), _VP, _VP, _VP]),
    "azp_bond_forces_quartic": (C.c_int, [C.POINTER(BondArgs), _VP, _VP, _VP]),
    "azp_special_pair_lj_params_make": (None, [_D] * 3 + [_VP]),
    "azp_special_pair_lj_params_unpack": (None, [_VP] + [_PD] * 3),
    "azp_special_pair_forces_lj": (C.c_int, [C.POINTER(PairGroupArgs), _VP, _VP]),
    "azp_angle_harmonic_params_make": (None, [_D] * 2 + [_VP]),
    "azp_angle_harmonic_params_unpack": (None, [_VP] + [_PD] * 2),
    "azp_angle_cossq_params_make": (None, [_D] * 2 + [_VP]),
    "azp_angle_cossq_params_unpack": (None, [_VP] + [_PD] * 2),
    "azp_angle_forces_harmonic": (C.c_int, [C.POINTER(AngleArgs), _VP, _VP]),
    "azp_angle_forces_cosine_squared": (C.c_int, [C.POINTER(AngleArgs), _VP, _VP]),
    "azp_dihedral_periodic_params_make": (None, [_D, C.c_int, C.c_uint, _D, _VP]),
    "azp_dihedral_periodic_params_unpack": (None, [_VP, _PD, _PI, C.POINTER(C.c_uint), _PD]),
    "azp_dihedral_opls_params_make": (None, [_D] * 4 + [_VP]),
    "azp_dihedral_opls_params_unpack": (None, [_VP] + [_PD] * 4),
    "azp_dihedral_forces_periodic": (C.c_int, [C.POINTER(DihedralArgs), _VP, _VP]),
    "azp_dihedral_forces_opls": (C.c_int, [C.POINTER(DihedralArgs), _VP, _VP]),
    "azp_angle_forces_table": (C.c_int, [C.POINTER(AngleArgs), _VP, _VP]),
    "azp_dihedral_forces_table": (C.c_int, [C.POINTER(DihedralArgs), _VP, _VP]),
    "azp_nlist_cell_assign": (C.c_int, [C.POINTER(NlistArgs), _VP]),
    "azp_nlist_cell_bounds": (C.c_int, [C.POINTER(NlistArgs), _VP]),
    "azp_nlist_bin": (C.c_int, [C.POINTER(NlistArgs), _VP, _VP, _VP]),
    "azp_nlist_count": (C.c_int, [C.POINTER(NlistArgs), _VP]),
    "azp_nlist_fill": (C.c_int, [C.POINTER(NlistArgs), _VP]),
    "azp_sorter_keys": (C.c_int, [C.c_uint32, _VP, C.POINTER(Box), C.POINTER(C.c_uint32), C.c_uint32, _VP, _VP]),
    "azp_halo_pack": (C.c_int, [C.c_uint32, _VP, _VP, C.c_uint32, _VP, _VP]),
    "azp_halo_pack_fields": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(HaloField), _VP, _VP, C.c_uint32, _VP]),
    "azp_halo_unpack_fields": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(HaloField), _VP, C.c_uint32, _VP]),
    "azp_nlist_distance_check": (C.c_int, [C.c_uint32, _VP, _VP, C.POINTER(Box), _D, _VP, _VP, _VP]),
    "azp_nlist_displacements": (C.c_int, [C.c_uint32, _VP, _VP, C.POINTER(Box), _D, _VP, _VP, _VP, _VP]),
    "azp_external_planar_harmonic_barrier": (C.c_int, [C.POINTER(BarrierArgs), _VP]),
    "azp_external_spherical_harmonic_barrier": (C.c_int, [C.POINTER(BarrierArgs), _VP]),
    "azp_planar_barrier_valid": (C.c_int, [_D, C.POINTER(Box)]),
    "azp_spherical_barrier_valid": (C.c_int, [_D, C.POINTER(Box)]),
    "azp_integrate_nve_step_one": (C.c_int, [C.POINTER(NVEArgs), _VP]),
    "azp_integrate_nve_step_two": (C.c_int, [C.POINTER(NVEArgs), _VP]),
    "azp_integrate_nve_step_two_one": (C.c_int, [C.POINTER(NVEArgs), _VP]),
    "azp_integrate_nve_rot_step_one": (C.c_int, [C.POINTER(NVERotArgs), _VP]),
    "azp_integrate_nve_rot_step_two": (C.c_int, [C.POINTER(NVERotArgs), _VP]),
    "azp_integrate_langevin_flow_step_one": (C.c_int, [C.POINTER(FlowMethodArgs), _VP]),
    "azp_integrate_langevin_flow_step_two": (C.c_int, [C.POINTER(FlowMethodArgs), _VP]),
    "azp_integrate_langevin_flow_step_two_one": (C.c_int, [C.POINTER(FlowMethodArgs), _VP]),
    "azp_integrate_brownian_flow_step": (C.c_int, [C.POINTER(FlowMethodArgs), _VP]),
    "azp_integrate_langevin_step_one": (C.c_int, [C.POINTER(LangevinArgs), _VP]),
    "azp_integrate_langevin_step_two": (C.c_int, [C.POINTER(LangevinArgs), _VP]),
    "azp_integrate_langevin_step_two_one": (C.c_int, [C.POINTER(LangevinArgs), _VP]),
    "azp_integrate_brownian_step": (C.c_int, [C.POINTER(LangevinArgs), _VP]),
    "azp_thermostat_partials_size": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint64)]),
    "azp_thermostat_kinetic": (C.c_int, [C.POINTER(ThermostatArgs), _VP]),
    "azp_thermostat_step_two": (C.c_int, [C.POINTER(ThermostatArgs), _VP]),
    "azp_thermostat_advance": (C.c_int, [C.POINTER(ThermostatArgs), _VP]),
    "azp_thermostat_step_one": (C.c_int, [C.POINTER(ThermostatArgs), _VP]),
    "azp_barostat_advance": (C.c_int, [C.POINTER(BarostatArgs), _VP]),
    "azp_barostat_step_one": (C.c_int, [C.POINTER(BarostatArgs), _VP]),
    "azp_barostat_step_two": (C.c_int, [C.POINTER(BarostatArgs), _VP]),
    "azp_fire_partials_size": (C.c_int, [C.c_uint32, C.POINTER(C.c_uint64)]),
    "azp_fire_measure": (C.c_int, [C.POINTER(FireArgs), _VP]),
    "azp_fire_step_two": (C.c_int, [C.POINTER(FireArgs), _VP]),
    "azp_fire_advance": (C.c_int, [C.POINTER(FireArgs), _VP]),
    "azp_fire_step_one": (C.c_int, [C.POINTER(FireArgs), _VP]),
    "azp_type_update_region": (C.c_int, [C.POINTER(TypeUpdateArgs), _VP]),
    "azp_box_resize": (C.c_int, [C.POINTER(BoxResizeArgs), _VP]),
    "azp_evaporate_scratch_size": (C.c_uint64, [C.c_uint32]),
    "azp_evaporate": (C.c_int, [C.POINTER(EvaporateArgs), _VP]),
    "azp_evaporate_local_keys": (C.c_int, [C.POINTER(EvaporateArgs), _VP]),
    "azp_evaporate_apply_below": (C.c_int, [C.POINTER(EvaporateArgs), C.c_uint64, _VP]),
    "azp_velocity_field_scratch_size": (C.c_int, [C.POINTER(VelocityFieldArgs), C.POINTER(C.c_uint64)]),
    "azp_velocity_field_sums": (C.c_int, [C.POINTER(VelocityFieldArgs), _VP]),
    "azp_velocity_field_normalize": (C.c_int, [_VP, C.c_uint64, _VP, _VP]),
    "azp_thermo_scratch_size": (C.c_int, [C.POINTER(ThermoArgs), C.POINTER(C.c_uint64)]),
    "azp_thermo_sums": (C.c_int, [C.POINTER(ThermoArgs), _VP]),
    "azp_thermo_field_scratch_size": (C.c_int, [C.POINTER(ThermoFieldArgs), C.POINTER(C.c_uint64)]),
    "azp_thermo_field_keys": (C.c_int, [C.POINTER(ThermoFieldArgs), _VP]),
    "azp_thermo_field_sums": (C.c_int, [C.POINTER(ThermoFieldArgs), _VP]),
    "azp_rdf_scratch_size": (C.c_int, [C.POINTER(RdfArgs), C.POINTER(C.c_uint64)]),
    "azp_rdf_counts": (C.c_int, [C.POINTER(RdfArgs), _VP]),
    "azp_rdf_subtract_excluded": (C.c_int, [C.POINTER(RdfExclusionArgs), _VP]),
    "azp_bonded_histogram": (C.c_int, [C.POINTER(BondedHistogramArgs), _VP]),
    "azp_pressure_profile_scratch_size": (C.c_int, [C.POINTER(PressureProfileArgs), C.POINTER(C.c_uint64)]),
    "azp_pressure_profile_begin": (C.c_int, [C.POINTER(PressureProfileArgs), _VP]),
    "azp_pressure_profile_pairs_perturbed_lennard_jones": (C.c_int, [C.POINTER(PressureProfileArgs), _VP, _VP]),
    "azp_pressure_profile_pairs_hertz": (C.c_int, [C.POINTER(PressureProfileArgs), _VP, _VP]),
    "azp_pressure_profile_pairs_expanded_yukawa": (C.c_int, [C.POINTER(PressureProfileArgs), _VP, _VP]),
    "azp_pressure_profile_pairs_colloid": (C.c_int, [C.POINTER(PressureProfileArgs), _VP, _VP]),
    "azp_pressure_profile_pairs_dpd_conservative": (C.c_int, [C.POINTER(PressureProfileArgs), _VP, _VP]),
    "azp_pressure_profile_pairs_table": (C.c_int, [C.POINTER(PressureProfileArgs), _VP, _VP]),
    "azp_pressure_profile_listed": (C.c_int, [C.POINTER(PressureProfileListArgs), _VP, _VP]),
    "azp_structure_factor_scratch_size": (C.c_int, [C.POINTER(StructureFactorArgs), C.POINTER(C.c_uint64)]),
    "azp_structure_factor_amplitudes": (C.c_int, [C.POINTER(StructureFactorArgs), _VP]),
    "azp_displacement_origin": (C.c_int, [C.POINTER(DisplacementOriginArgs), _VP]),
    "azp_displacement_moments_scratch_size": (C.c_int, [C.POINTER(DisplacementArgs), C.POINTER(C.c_uint64)]),
    "azp_displacement_moments": (C.c_int, [C.POINTER(DisplacementArgs), _VP]),
    "azp_self_scattering_scratch_size": (C.c_int, [C.POINTER(DisplacementArgs), C.POINTER(C.c_uint64)]),
    "azp_self_scattering": (C.c_int, [C.POINTER(DisplacementArgs), _VP]),
    "azp_steinhardt_scratch_size": (C.c_int, [C.POINTER(SteinhardtArgs), C.POINTER(C.c_uint64)]),
    "azp_steinhardt_compute": (C.c_int, [C.POINTER(SteinhardtArgs), _VP]),
    "azp_cluster_scratch_size": (C.c_int, [C.POINTER(ClusterArgs), C.POINTER(C.c_uint64)]),
    "azp_cluster_compute": (C.c_int, [C.POINTER(ClusterArgs), _VP]),
    "azp_cluster_properties_scratch_size": (C.c_int, [C.POINTER(ClusterPropertiesArgs), C.POINTER(C.c_uint64)]),
    "azp_cluster_properties": (C.c_int, [C.POINTER(ClusterPropertiesArgs), _VP]),
    "azp_wall_lj93_params_make": (C.c_int, [_D] * 4 + [C.c_int, _PD]),
    "azp_wall_colloid_params_make": (C.c_int, [_D] * 5 + [C.c_int, _PD]),
    "azp_wall_forces_lj93": (C.c_int, [C.POINTER(WallArgs), _VP]),
    "azp_wall_forces_colloid": (C.c_int, [C.POINTER(WallArgs), _VP]),
    "azp_wall_net_forces_scratch_size": (C.c_int, [C.POINTER(WallArgs), C.POINTER(C.c_uint64)]),
    "azp_wall_net_forces_lj93": (C.c_int, [C.POINTER(WallArgs), _VP, _VP, C.c_uint64, _VP]),
    "azp_wall_net_forces_colloid": (C.c_int, [C.POINTER(WallArgs), _VP, _VP, C.c_uint64, _VP]),
    "azp_version": (C.c_int, []),
    "azp_status_string": (C.c_char_p, [C.c_int]),
    "azp_last_launch": (None, [C.POINTER(C.c_uint32)] * 4),
}

_lib = None


def lib():
    """Load libazp.so; raise (never fall back) if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AzpError(
                "libazp.so not found at %s: build it with `make -C %s` (or __graft_entry__.build()); "
                "there is no CPU fallback" % (LIB_PATH, CSRC)
            )
        # One HIP runtime per process: torch ships its own libamdhip64.so.7 and
        # must be loaded first so that libazp binds to the same runtime (the
        # device pointers and streams handed across the C ABI are torch's).
        import torch  # noqa: F401

        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


_ext = None


def ext_module():
    """The compiled ``_azplugins`` module (pybind11, built by ``make -C csrc``): the class
    names the reference registers (src/module.cc:110-166), holding the host-side parameter
    tables in C++. libazp (and with it torch's HIP runtime) is loaded first."""
    global _ext
    if _ext is None:
        lib()
        try:
            from . import _azplugins as m
        except ImportError as e:
            raise AzpError("the _azplugins extension module is missing (%s): build it with `make -C %s`" % (e, CSRC))
        _ext = m
    return _ext


def check(rc, what="libazp call"):
    if rc != 0:
        msg = lib().azp_status_string(rc).decode()
        raise AzpError("%s failed: status %d (%s)" % (what, rc, msg))


def table_pack(r_min, r_end, U, F, closed):
    """azp_table_pack: the rows {U_k, U_{k+1} - U_k, F_k, F_{k+1} - F_k} of one table (numpy, n x 4), or None for
    input the library refuses."""
    import numpy as np

    U = np.ascontiguousarray(U, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.float64)
    if U.ndim != 1 or U.shape != F.shape:
        return None
    rows = np.zeros((max(len(U) - (1 if closed else 0), 0), 4))
    rc = lib().azp_table_pack(float(r_min), float(r_end), U.ctypes.data, F.ctypes.data, len(U), 1 if closed else 0, rows.ctypes.data)
    return rows if rc == 0 else None


def table_params_rows(entries):
    """The azp_table_params structs ``(r_min, r_max, device address of the rows, n)`` of ``entries`` as float64 words
    (len(entries) x 4), the form the parameter tables are uploaded in."""
    import numpy as np

    arr = (TableParams * max(len(entries), 1))()
    for p, (r_min, r_max, ptr, n) in zip(arr, entries):
        p.r_min, p.r_max, p.d_rows, p.n = r_min, r_max, ptr, n
    return np.frombuffer(bytes(arr), dtype=np.float64).reshape(-1, 4).copy()


def raw_stream(device):
    """The current HIP stream of ``device`` as an integer handle (what the C ABI takes);
    torch.cuda.current_stream(device).cuda_stream without the Stream object (4 us per launch)."""
    import torch

    try:
        idx = device.index if isinstance(device, torch.device) else torch.device(device).index
        return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device() if idx is None else idx)
    except AttributeError:  # private hook missing in this torch build
        return torch.cuda.current_stream(device).cuda_stream


def make_box(L, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    b = Box()
    try:
        L = (float(L),) * 3
    except TypeError:
        pass
    for k in range(3):
        b.L[k] = float(L[k])
        b.tilt[k] = float(tilt[k])
        b.periodic[k] = int(periodic[k])
    return b


class PairPlan:
    """Owner of one azp_pair_plan handle."""

    def __init__(self):
        self._h = _VP()
        check(lib().azp_pair_plan_create(C.byref(self._h)), "azp_pair_plan_create")

    def build(self, args, stream):
        check(lib().azp_pair_plan_build(self._h, C.byref(args), stream), "azp_pair_plan_build")

    def build_from_cells(self, cells, pair, stream):
        check(lib().azp_pair_plan_build_from_cells(self._h, C.byref(cells), C.byref(pair), stream), "azp_pair_plan_build_from_cells")

    def tile_stage(self):
        """Staged-set size of every tile of the last build (numpy uint32)."""
        import numpy as np

        n = self.info()["n_tiles"]
        out = np.zeros(max(n, 1), dtype=np.uint32)
        m = lib().azp_pair_plan_tile_stage(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n)
        return out[:max(m, 0)]

    def set_balance(self, enabled):
        check(lib().azp_pair_plan_set_balance(self._h, int(bool(enabled))), "azp_pair_plan_set_balance")

    def set_bank_order(self, enabled):
        check(lib().azp_pair_plan_set_bank_order(self._h, int(bool(enabled))), "azp_pair_plan_set_bank_order")

    def info(self):
        i = PlanInfo()
        check(lib().azp_pair_plan_query(self._h, C.byref(i)), "azp_pair_plan_query")
        return {f[0]: getattr(i, f[0]) for f in PlanInfo._fields_ if f[0] != "_pad"}

    def phase_chunks(self):
        """Diagnostics: mean chunks per slice covering the core entries / up to the end of the all-sure part / whole rows."""
        out = (C.c_float * 3)()
        check(lib().azp_pair_plan_phase_chunks(self._h, out), "azp_pair_plan_phase_chunks")
        return [float(x) for x in out]

    def row_batches(self):
        """Row ends of the last build: (counts, shell width). counts[slice, 0] batches of 4 entries per lane covering
        the in-range entries, counts[slice, 1 + s] up to the end of buffer shell s; the last column is the whole row."""
        import numpy as np

        cols = int(lib().azp_pair_plan_shells()) + 1
        out = np.zeros(max(4 * self.info()["n_tiles"], 1) * cols, dtype=np.uint32)
        w = C.c_double(0.0)
        m = lib().azp_pair_plan_row_batches(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(w))
        if m < 0:
            check(m, "azp_pair_plan_row_batches")
        return out[:m].reshape(-1, cols), w.value

    @property
    def handle(self):
        return self._h

    def __del__(self):
        try:
            if self._h:
                lib().azp_pair_plan_destroy(self._h)
                self._h = None
        except Exception:
            pass


def auto_plan_stats():
    """Counters of the plan cache behind the HOOMD-signature entry points."""
    st = AutoPlanStats()
    lib().azp_pair_auto_plan_get_stats(C.byref(st))
    return {f[0]: int(getattr(st, f[0])) for f in AutoPlanStats._fields_}


def last_launch():
    vals = [C.c_uint32(0) for _ in range(4)]
    lib().azp_last_launch(*[C.byref(v) for v in vals])
    return dict(block_size=vals[0].value, threads_per_particle=vals[1].value, grid=vals[2].value,
                lds_bytes=vals[3].value)
