"""ctypes mirror of ``include/neutral_hip.h`` (libneutral_hip.so).

The three functions keep the reference's names, argument order and meaning
(``neutral_interface.h:11-36``); ``Simulation`` is a thin convenience that keeps
the device buffers of one problem together, the way ``main.c`` keeps them in
``Mesh``/``SharedData``/``NeutralData``.

There is no CPU fallback: if the HIP library is missing, importing this module
raises.  Device buffers are torch CUDA tensors (PyTorch is used for device
memory, streams and ``torch.distributed`` only); particle arrays are allocated
by the library's own ``inject_particles`` as in the reference.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
# torch must be imported before libneutral_hip.so is loaded: the PyTorch-ROCm
# wheel bundles its own libamdhip64, and one process must hold exactly one HIP
# runtime (loading the system one first makes every later device call fail).
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# NEUTRAL_HIP_LIB selects another build of the same ABI (kernel experiments)
LIB_PATH = os.environ.get("NEUTRAL_HIP_LIB") or os.path.join(_HERE, "libneutral_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} has not been built (run __graft_entry__.build() or "
        "`make -C neutral_amd`); neutral_amd has no CPU fallback")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_u64p = C.POINTER(C.c_uint64)

VARIANT_OVER_PARTICLE = 0
VARIANT_EVENT_SORTED = 1
VARIANT_TILED = 2

F64_FIELDS = ("x", "y", "omega_x", "omega_y", "energy", "weight", "dt_to_census",
              "mfp_to_collision")
I32_FIELDS = ("cellx", "celly", "dead")


class CrossSection(C.Structure):
    """neutral_data.h:38-43"""
    _fields_ = [("keys", C.c_void_p), ("values", C.c_void_p), ("nentries", C.c_int)]


class Particle(C.Structure):
    """neutral_data.h:45-61 (-DSoA): host struct of device arrays"""
    _fields_ = [(n, C.c_void_p) for n in F64_FIELDS + I32_FIELDS]


class StepStats(C.Structure):
    _fields_ = [("nprocessed", C.c_uint64), ("facets", C.c_uint64),
                ("collisions", C.c_uint64), ("census", C.c_uint64),
                ("kernel_ms", C.c_double),
                ("same_tables", C.c_int), ("variant", C.c_int),
                ("sort_ms", C.c_double), ("stream_ms", C.c_double),
                ("collide_ms", C.c_double), ("stream_facets", C.c_uint64),
                ("stream_census", C.c_uint64), ("suspended", C.c_uint64),
                ("aborted", C.c_uint64), ("stream_passes", C.c_int),
                ("requeued", C.c_uint64), ("collide_passes", C.c_uint64),
                ("host_syncs", C.c_int), ("stream_passes_enqueued", C.c_int),
                ("tile_cells", C.c_int), ("export_ms", C.c_double),
                ("checked_arithmetic", C.c_int), ("attempts", C.c_int),
                ("host_collectives", C.c_int), ("exchange_ranks", C.c_int),
                ("steals", C.c_uint64), ("steals_refused", C.c_uint64),
                ("stream_hops", C.c_uint64), ("stream_overflows", C.c_uint64),
                ("stream_batches", C.c_uint64), ("stream_idle_polls", C.c_uint64),
                ("local_nprocessed", C.c_uint64), ("exchange_ms", C.c_double),
                ("exchange_rounds", C.c_int), ("emigrants", C.c_uint64),
                ("weighted_waves", C.c_uint64),
                ("stream_clock_ghz", C.c_double), ("collide_clock_ghz", C.c_double),
                ("roulette_killed", C.c_uint64), ("roulette_survived", C.c_uint64),
                ("roulette_weight_lost", C.c_double), ("roulette_weight_gained", C.c_double)]


class CombStats(C.Structure):
    """NeutralHipCombStats: what one census weight comb found and did"""
    _fields_ = [("live_before", C.c_uint64), ("sources_kept", C.c_uint64),
                ("max_copies", C.c_uint64), ("weight_before", C.c_double),
                ("weight_each", C.c_double), ("comb_ms", C.c_double)]


class SourceStats(C.Structure):
    """NeutralHipSourceStats: what one call of the fixed source found and did"""
    _fields_ = [("dead_before", C.c_uint64), ("emitted", C.c_uint64),
                ("weight_emitted", C.c_double), ("source_ms", C.c_double)]


SOURCE_MAX_COMPONENTS, SOURCE_MAX_BINS = 16, 256


class SourceComponentC(C.Structure):
    """NeutralHipSourceComponent: one component of a described source, as the library takes it"""
    _fields_ = [("share", C.c_double), ("left", C.c_double), ("bottom", C.c_double),
                ("width", C.c_double), ("height", C.c_double), ("theta0", C.c_double),
                ("theta_width", C.c_double), ("bin_first", C.c_int), ("bin_count", C.c_int)]


class SourceBinC(C.Structure):
    """NeutralHipSourceBin: one energy bin of a described source (e_lo == e_hi: a line)"""
    _fields_ = [("e_lo", C.c_double), ("e_hi", C.c_double), ("share", C.c_double)]


class DescribedSourceStats(C.Structure):
    """NeutralHipDescribedSourceStats: what one call of the described source found and did"""
    _fields_ = [("dead_before", C.c_uint64), ("emitted", C.c_uint64),
                ("emitted_by_component", C.c_uint64 * SOURCE_MAX_COMPONENTS),
                ("weight_emitted", C.c_double), ("source_ms", C.c_double)]


class MeshSourceStats(C.Structure):
    """NeutralHipMeshSourceStats: what one call of the mesh source found and did"""
    _fields_ = [("dead_before", C.c_uint64), ("emitted", C.c_uint64), ("cells_nonzero", C.c_uint64),
                ("strength_total", C.c_double), ("weight_emitted", C.c_double), ("source_ms", C.c_double)]


class WindowStats(C.Structure):
    """NeutralHipWindowStats: what one call of the census weight window found and did"""
    _fields_ = [("live_before", C.c_uint64), ("dead_before", C.c_uint64), ("below", C.c_uint64),
                ("roulette_killed", C.c_uint64), ("roulette_survived", C.c_uint64),
                ("above", C.c_uint64), ("split", C.c_uint64), ("copies_made", C.c_uint64),
                ("copies_refused", C.c_uint64), ("roulette_weight_lost", C.c_double),
                ("roulette_weight_gained", C.c_double), ("window_ms", C.c_double)]


class CensusStats(C.Structure):
    """NeutralHipCensusStats: what one census tally found"""
    _fields_ = [("live", C.c_uint64), ("dead", C.c_uint64), ("occupied_cells", C.c_uint64),
                ("max_count", C.c_uint64), ("weight", C.c_double), ("max_cell_weight", C.c_double),
                ("census_ms", C.c_double)]


class GroupCensusStats(C.Structure):
    """NeutralHipGroupCensusStats: what one census tally over (cell, energy group) bins found"""
    _fields_ = [("live", C.c_uint64), ("dead", C.c_uint64), ("outside", C.c_uint64),
                ("occupied_bins", C.c_uint64), ("max_count", C.c_uint64), ("weight", C.c_double),
                ("max_bin_weight", C.c_double), ("census_ms", C.c_double)]


class GroupWindowStats(C.Structure):
    """NeutralHipGroupWindowStats: what one call of the grouped weight window found and did --
    the plain window's stats and the live slots in no group"""
    _fields_ = [("window", WindowStats), ("outside", C.c_uint64)]


class BlockCensusStats(C.Structure):
    """NeutralHipBlockCensusStats: what one census tally over blocks of cells found -- the grouped
    census's stats (outside 0 without groups) and whether the pass summed its bins in LDS"""
    _fields_ = [("census", GroupCensusStats), ("privatised", C.c_uint64)]


class BoundsStats(C.Structure):
    """NeutralHipBoundsStats: what one call of the window bounds made"""
    _fields_ = [("windowed_cells", C.c_uint64), ("floored_cells", C.c_uint64),
                ("max_cell_weight", C.c_double), ("lower_at_peak", C.c_double),
                ("bounds_ms", C.c_double)]


class BatchFoldStats(C.Structure):
    """NeutralHipBatchFoldStats: what one fold of a batch into the running moments found"""
    _fields_ = [("sum", C.c_double), ("nonzero", C.c_uint64), ("fold_ms", C.c_double)]


class BatchStats(C.Structure):
    """NeutralHipBatchStats: the relative errors of the scored entries, in numbers"""
    _fields_ = [("scored", C.c_uint64), ("within_10pc", C.c_uint64), ("within_5pc", C.c_uint64),
                ("max_relerr", C.c_double), ("mean_relerr", C.c_double), ("estimate_sum", C.c_double),
                ("stats_ms", C.c_double)]


class EscapeStats(C.Structure):
    """NeutralHipEscapeStats: the last step's escapes through vacuum sides, by the outflow tally's
    side number (west, east, south, north), and the sum of the weights they left with."""
    _fields_ = [("escaped", C.c_uint64 * 4), ("weight", C.c_double * 4)]

    def counts(self):
        return tuple(int(v) for v in self.escaped)

    def weights(self):
        return tuple(float(v) for v in self.weight)


class WrapStats(C.Structure):
    """NeutralHipWrapStats: the last step's wraps through periodic axes, by the side the histories
    LEFT through (the outflow tally's numbers: west, east, south, north), and the sum of the weights
    they wrapped with."""
    _fields_ = [("wrapped", C.c_uint64 * 4), ("weight", C.c_double * 4)]

    def counts(self):
        return tuple(int(v) for v in self.wrapped)

    def weights(self):
        return tuple(float(v) for v in self.weight)


class EscapeRecord(C.Structure):
    """NeutralHipEscapeRecord: one escaped history as the escape bank keeps it (64 bytes)"""
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("omega_x", C.c_double), ("omega_y", C.c_double),
                ("energy", C.c_double), ("weight", C.c_double), ("time_left", C.c_double),
                ("slot", C.c_uint32), ("side", C.c_uint32)]


assert C.sizeof(EscapeRecord) == 64
# ... and as numpy sees a bank: a structured array of the same 64 bytes
ESCAPE_RECORD = np.dtype([("x", "<f8"), ("y", "<f8"), ("omega_x", "<f8"), ("omega_y", "<f8"), ("energy", "<f8"),
                          ("weight", "<f8"), ("time_left", "<f8"), ("slot", "<u4"), ("side", "<u4")])
assert ESCAPE_RECORD.itemsize == 64


class EscapeBankStats(C.Structure):
    """NeutralHipEscapeBankStats: the bank's capacity, its cursor, what it holds, and the last step's share"""
    _fields_ = [("capacity", C.c_uint64), ("claimed", C.c_uint64), ("recorded", C.c_uint64),
                ("step_claimed", C.c_uint64), ("step_recorded", C.c_uint64)]


class BankSourceStats(C.Structure):
    """NeutralHipBankSourceStats: what one call of the bank source found and did"""
    _fields_ = [("dead_before", C.c_uint64), ("emitted", C.c_uint64), ("snapped", C.c_uint64),
                ("first_bad", C.c_uint64), ("weight_emitted", C.c_double), ("source_ms", C.c_double)]


# every symbol include/neutral_hip.h declares
ABI_SYMBOLS = (
    "solve_transport_2d", "inject_particles", "validate",
    "allocate_data", "allocate_float_data", "allocate_int_data", "allocate_uint64_data",
    "allocate_host_data", "allocate_host_int_data", "deallocate_data",
    "deallocate_int_data", "deallocate_uint64_data", "deallocate_host_data",
    "copy_buffer", "copy_int_buffer", "move_host_buffer_to_device",
    "neutral_hip_device_count", "neutral_hip_set_device", "neutral_hip_set_stream",
    "neutral_hip_set_pid_base", "neutral_hip_get_pid_base", "neutral_hip_set_variant",
    "neutral_hip_set_quiet", "neutral_hip_set_tests_file", "neutral_hip_last_step",
    "neutral_hip_set_arithmetic",
    "neutral_hip_reinject_particles", "neutral_hip_free_particles",
    "neutral_hip_set_lazy_export", "neutral_hip_set_stream_queues", "neutral_hip_sync_particles",
    "neutral_hip_invalidate_particles", "neutral_hip_set_scalar_flux_tally",
    "neutral_hip_set_collision_tallies", "neutral_hip_set_roulette",
    "neutral_hip_set_spectrum_tally", "neutral_hip_set_current_tally",
    "neutral_hip_set_outflow_tally", "neutral_hip_comb_particles",
    "neutral_hip_source_particles", "neutral_hip_source_described", "neutral_hip_source_mesh",
    "neutral_hip_window_particles",
    "neutral_hip_census_tally", "neutral_hip_window_bounds",
    "neutral_hip_census_tally_groups", "neutral_hip_window_particles_groups",
    "neutral_hip_census_tally_blocks", "neutral_hip_window_particles_blocks",
    "neutral_hip_set_window_roulette",
    "neutral_hip_set_vacuum_sides", "neutral_hip_get_vacuum_sides", "neutral_hip_last_escape",
    "neutral_hip_set_periodic_axes", "neutral_hip_get_periodic_axes", "neutral_hip_last_wraps",
    "neutral_hip_set_leakage_tally",
    "neutral_hip_set_escape_bank", "neutral_hip_reset_escape_bank", "neutral_hip_escape_bank_stats",
    "neutral_hip_source_bank",
    "neutral_hip_batch_fold", "neutral_hip_batch_statistics",
    "neutral_hip_comm_start", "neutral_hip_comm_stop", "neutral_hip_comm_rank",
    "neutral_hip_comm_nranks", "neutral_hip_comm_transport", "neutral_hip_comm_rccl_version",
    "neutral_hip_set_auto_shard",
    "neutral_hip_store_count", "neutral_hip_set_decomposition",
    "neutral_hip_clear_decomposition", "neutral_hip_set_source_box", "neutral_hip_store_keys",
    "neutral_hip_comm_allreduce_f64", "neutral_hip_comm_max",
    "neutral_hip_comm_barrier", "neutral_hip_bind_rank_device",
    "neutral_hip_comm_barrier_device", "neutral_hip_comm_selftest",
    "neutral_hip_memcpy_d2h", "neutral_hip_memcpy_h2d", "neutral_hip_memset",
    "neutral_hip_synchronize", "neutral_hip_abi_version",
    "neutral_hip_probe_threefry", "neutral_hip_probe_cs_lookup",
    "neutral_hip_probe_distance_to_facet", "neutral_hip_probe_division", "neutral_hip_probe_scatter",
    "neutral_hip_probe_log", "neutral_hip_probe_policy_quotient", "neutral_hip_probe_policy_root",
)

_lib = C.CDLL(LIB_PATH)

_lib.solve_transport_2d.restype = None
_lib.solve_transport_2d.argtypes = [
    C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int,
    C.c_double, C.c_int, _ip, C.c_void_p, C.POINTER(Particle), C.c_void_p,
    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CrossSection),
    C.POINTER(CrossSection), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
    _u64p, _u64p]
_lib.inject_particles.restype = C.c_size_t
_lib.inject_particles.argtypes = [
    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
    C.c_double, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_double,
    C.POINTER(C.POINTER(Particle))]
_lib.validate.restype = None
_lib.validate.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_void_p]
_lib.neutral_hip_device_count.restype = C.c_int
_lib.neutral_hip_set_device.restype = C.c_int
_lib.neutral_hip_set_device.argtypes = [C.c_int]
_lib.neutral_hip_set_stream.argtypes = [C.c_void_p]
_lib.neutral_hip_set_pid_base.argtypes = [C.c_uint64]
_lib.neutral_hip_get_pid_base.restype = C.c_uint64
_lib.neutral_hip_set_variant.restype = C.c_int
_lib.neutral_hip_set_variant.argtypes = [C.c_int]
_lib.neutral_hip_set_quiet.argtypes = [C.c_int]
_lib.neutral_hip_set_arithmetic.restype = C.c_int
_lib.neutral_hip_set_arithmetic.argtypes = [C.c_int]
_lib.neutral_hip_set_tests_file.argtypes = [C.c_char_p]
_lib.neutral_hip_last_step.argtypes = [C.POINTER(StepStats)]
_lib.neutral_hip_reinject_particles.restype = None
_lib.neutral_hip_reinject_particles.argtypes = [
    C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
    C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(Particle)]
_lib.neutral_hip_free_particles.argtypes = [C.POINTER(Particle)]
_lib.neutral_hip_set_lazy_export.argtypes = [C.c_int]
_lib.neutral_hip_sync_particles.argtypes = [C.POINTER(Particle)]
_lib.neutral_hip_invalidate_particles.argtypes = [C.POINTER(Particle)]
_lib.neutral_hip_set_scalar_flux_tally.argtypes = [C.c_void_p]
_lib.neutral_hip_set_collision_tallies.restype = C.c_int
_lib.neutral_hip_set_collision_tallies.argtypes = [C.c_void_p, C.c_void_p]
_lib.neutral_hip_set_current_tally.restype = C.c_int
_lib.neutral_hip_set_current_tally.argtypes = [C.c_void_p, C.c_void_p]
if hasattr(_lib, "neutral_hip_set_outflow_tally"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_set_outflow_tally.restype = None
    _lib.neutral_hip_set_outflow_tally.argtypes = [C.c_void_p]
if hasattr(_lib, "neutral_hip_set_vacuum_sides"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_set_vacuum_sides.restype = C.c_int
    _lib.neutral_hip_set_vacuum_sides.argtypes = [C.c_uint]
    _lib.neutral_hip_get_vacuum_sides.restype = C.c_uint
    _lib.neutral_hip_get_vacuum_sides.argtypes = []
    _lib.neutral_hip_last_escape.restype = None
    _lib.neutral_hip_last_escape.argtypes = [C.POINTER(EscapeStats)]
if hasattr(_lib, "neutral_hip_set_periodic_axes"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_set_periodic_axes.restype = C.c_int
    _lib.neutral_hip_set_periodic_axes.argtypes = [C.c_uint]
    _lib.neutral_hip_get_periodic_axes.restype = C.c_uint
    _lib.neutral_hip_get_periodic_axes.argtypes = []
    _lib.neutral_hip_last_wraps.restype = None
    _lib.neutral_hip_last_wraps.argtypes = [C.POINTER(WrapStats)]
if hasattr(_lib, "neutral_hip_set_leakage_tally"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_set_leakage_tally.restype = C.c_int
    _lib.neutral_hip_set_leakage_tally.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.c_void_p]
if hasattr(_lib, "neutral_hip_set_escape_bank"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_set_escape_bank.restype = C.c_int
    _lib.neutral_hip_set_escape_bank.argtypes = [C.c_void_p, C.c_uint64]
    _lib.neutral_hip_reset_escape_bank.restype = C.c_int
    _lib.neutral_hip_reset_escape_bank.argtypes = []
    _lib.neutral_hip_escape_bank_stats.restype = None
    _lib.neutral_hip_escape_bank_stats.argtypes = [C.POINTER(EscapeBankStats)]
    _lib.neutral_hip_source_bank.restype = C.c_int
    _lib.neutral_hip_source_bank.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_double, C.POINTER(C.c_double),
        C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
        C.POINTER(BankSourceStats)]
_lib.neutral_hip_comb_particles.restype = C.c_int
_lib.neutral_hip_comb_particles.argtypes = [C.POINTER(Particle), C.c_int, C.c_uint64,
                                            C.POINTER(CombStats)]
if hasattr(_lib, "neutral_hip_source_particles"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_source_particles.restype = C.c_int
    _lib.neutral_hip_source_particles.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_double, C.c_uint64,
        C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
        C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(SourceStats)]
if hasattr(_lib, "neutral_hip_source_described"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_source_described.restype = C.c_int
    _lib.neutral_hip_source_described.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_double, C.c_uint64,
        C.c_int, C.POINTER(SourceComponentC), C.c_int, C.POINTER(SourceBinC),
        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
        C.POINTER(DescribedSourceStats)]
if hasattr(_lib, "neutral_hip_source_mesh"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_source_mesh.restype = C.c_int
    _lib.neutral_hip_source_mesh.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_double, C.c_uint64,
        C.c_void_p, C.c_double, C.c_double, C.c_int, C.POINTER(SourceBinC),
        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
        C.POINTER(MeshSourceStats)]
if hasattr(_lib, "neutral_hip_window_particles"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_window_particles.restype = C.c_int
    _lib.neutral_hip_window_particles.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_int,
        C.c_uint64, C.POINTER(WindowStats)]
if hasattr(_lib, "neutral_hip_census_tally"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_census_tally.restype = C.c_int
    _lib.neutral_hip_census_tally.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(CensusStats)]
if hasattr(_lib, "neutral_hip_census_tally_groups"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_census_tally_groups.restype = C.c_int
    _lib.neutral_hip_census_tally_groups.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p,
        C.POINTER(GroupCensusStats)]
    _lib.neutral_hip_window_particles_groups.restype = C.c_int
    _lib.neutral_hip_window_particles_groups.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_void_p,
        C.c_double, C.c_double, C.c_int, C.c_uint64, C.POINTER(GroupWindowStats)]
if hasattr(_lib, "neutral_hip_census_tally_blocks"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_census_tally_blocks.restype = C.c_int
    _lib.neutral_hip_census_tally_blocks.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
        C.c_void_p, C.POINTER(BlockCensusStats)]
    _lib.neutral_hip_window_particles_blocks.restype = C.c_int
    _lib.neutral_hip_window_particles_blocks.argtypes = [
        C.POINTER(Particle), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
        C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_uint64, C.POINTER(GroupWindowStats)]
if hasattr(_lib, "neutral_hip_set_window_roulette"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_set_window_roulette.restype = C.c_int
    _lib.neutral_hip_set_window_roulette.argtypes = [
        C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int]
if hasattr(_lib, "neutral_hip_window_bounds"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_window_bounds.restype = C.c_int
    _lib.neutral_hip_window_bounds.argtypes = [
        C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p,
        C.POINTER(BoundsStats)]
if hasattr(_lib, "neutral_hip_batch_fold"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_batch_fold.restype = C.c_int
    _lib.neutral_hip_batch_fold.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p,
                                            C.POINTER(BatchFoldStats)]
    _lib.neutral_hip_batch_statistics.restype = C.c_int
    _lib.neutral_hip_batch_statistics.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_void_p,
                                                  C.c_void_p, C.POINTER(BatchStats)]
_lib.neutral_hip_set_roulette.restype = C.c_int
_lib.neutral_hip_set_spectrum_tally.restype = C.c_int
_lib.neutral_hip_set_spectrum_tally.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_void_p]
_lib.neutral_hip_set_roulette.argtypes = [C.c_double, C.c_double]
_lib.neutral_hip_comm_start.restype = C.c_int
_lib.neutral_hip_comm_rank.restype = C.c_int
_lib.neutral_hip_comm_nranks.restype = C.c_int
_lib.neutral_hip_comm_transport.restype = C.c_int
_lib.neutral_hip_set_auto_shard.argtypes = [C.c_int]
_lib.neutral_hip_store_count.restype = C.c_int
_lib.neutral_hip_store_count.argtypes = [C.POINTER(Particle)]
_lib.neutral_hip_set_decomposition.restype = C.c_int
_lib.neutral_hip_set_decomposition.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip, _ip]
_lib.neutral_hip_set_source_box.argtypes = [C.c_double] * 4
_lib.neutral_hip_store_keys.restype = C.c_void_p
_lib.neutral_hip_store_keys.argtypes = [C.POINTER(Particle)]
_lib.neutral_hip_comm_allreduce_f64.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
if hasattr(_lib, "neutral_hip_comm_rccl_version"):   # (absent from older builds: same-box A/B runs)
    _lib.neutral_hip_comm_rccl_version.restype = C.c_int
_lib.neutral_hip_comm_max.restype = C.c_double
_lib.neutral_hip_comm_max.argtypes = [C.c_double]
_lib.neutral_hip_bind_rank_device.argtypes = [C.c_int]
_lib.neutral_hip_comm_selftest.restype = C.c_int
_lib.neutral_hip_comm_selftest.argtypes = [C.c_int]

COMM_NONE, COMM_RCCL, COMM_HOST = 0, 1, 2
_lib.neutral_hip_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
_lib.neutral_hip_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
_lib.neutral_hip_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
_lib.neutral_hip_abi_version.restype = C.c_int
_lib.neutral_hip_probe_threefry.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
_lib.neutral_hip_probe_cs_lookup.argtypes = [C.POINTER(CrossSection), C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_int]
_lib.neutral_hip_probe_division.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
_lib.neutral_hip_probe_scatter.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
_lib.neutral_hip_probe_log.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
_lib.neutral_hip_probe_policy_quotient.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
_lib.neutral_hip_probe_policy_root.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
_lib.neutral_hip_probe_distance_to_facet.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_int]


def library() -> C.CDLL:
    return _lib


# ---- the three interface functions, reference names and argument order ---------

def solve_transport_2d(nx, ny, global_nx, global_ny, master_key, pad, x_off, y_off, dt,
                       ntotal_particles, nlocal_particles, neighbours, particles, density,
                       edgex, edgey, edgedx, edgedy, cs_scatter_table, cs_absorb_table,
                       energy_deposition_tally, reduce_array0, reduce_array1,
                       reduce_array2, facet_events, collision_events):
    """neutral_interface.h:11-20.  Pointer arguments are device addresses (ints)
    or ctypes objects; `nlocal_particles`, `facet_events`, `collision_events` are
    ctypes scalars passed by reference like the C int*/uint64_t*."""
    _lib.solve_transport_2d(nx, ny, global_nx, global_ny, master_key, pad, x_off, y_off,
                            dt, ntotal_particles, C.byref(nlocal_particles), neighbours,
                            particles, density, edgex, edgey, edgedx, edgedy,
                            C.byref(cs_scatter_table), C.byref(cs_absorb_table),
                            energy_deposition_tally, reduce_array0, reduce_array1,
                            reduce_array2, C.byref(facet_events), C.byref(collision_events))


def inject_particles(nparticles, global_nx, local_nx, local_ny, pad,
                     local_particle_left_off, local_particle_bottom_off,
                     local_particle_width, local_particle_height, x_off, y_off, dt,
                     edgex, edgey, initial_energy):
    """neutral_interface.h:23-31.  Returns (particles, bytes_allocated), where
    `particles` is the C `Particle*` the library allocated."""
    pp = C.POINTER(Particle)()
    nbytes = _lib.inject_particles(nparticles, global_nx, local_nx, local_ny, pad,
                                   local_particle_left_off, local_particle_bottom_off,
                                   local_particle_width, local_particle_height, x_off,
                                   y_off, dt, edgex, edgey, initial_energy, C.byref(pp))
    return pp, nbytes


def validate(nx, ny, params_filename, rank, energy_tally):
    """neutral_interface.h:35-36 (prints; returns nothing, like the reference)."""
    _lib.validate(nx, ny, params_filename.encode(), rank, energy_tally)


# ---- extensions -------------------------------------------------------------------

def device_count() -> int:
    return _lib.neutral_hip_device_count()


def set_device(device: int) -> None:
    if _lib.neutral_hip_set_device(device) != 0:
        raise RuntimeError(f"hipSetDevice({device}) failed")


def set_stream(stream_handle: int) -> None:
    _lib.neutral_hip_set_stream(C.c_void_p(stream_handle))


def set_pid_base(pid_base: int) -> None:
    _lib.neutral_hip_set_pid_base(pid_base)


def set_variant(variant: int) -> None:
    if _lib.neutral_hip_set_variant(variant) != 0:
        raise ValueError(f"unknown kernel variant {variant}")


def _device_address(a):
    """None, an integer device address, or a float64 torch tensor on a GPU (its storage)."""
    if a is None:
        return None
    if isinstance(a, int):
        return a or None
    if hasattr(a, "data_ptr"):
        if str(a.dtype) != "torch.float64":
            raise TypeError(f"a tally mesh is float64, not {a.dtype}")
        if not a.is_contiguous():
            raise ValueError("a tally mesh must be contiguous")
        return a.data_ptr()
    raise TypeError(f"not a device array: {type(a).__name__}")


def set_collision_tallies(collisions=None, absorbed=None) -> None:
    """The collision tallies of the following steps (include/neutral_hip.h): two meshes of
    ny*nx doubles in device memory, given as float64 tensors or device addresses; both None
    (the default) turns them off.  One without the other is refused."""
    c, a = _device_address(collisions), _device_address(absorbed)
    if (c is None) != (a is None):
        raise ValueError("the collision tallies are kept both or neither")
    if _lib.neutral_hip_set_collision_tallies(c, a) != 0:
        raise ValueError("the collision tallies are kept both or neither")


def set_current_tally(jx=None, jy=None) -> None:
    """The net current of the following steps (include/neutral_hip.h): Jx and Jy per cell, two
    meshes of ny*nx doubles in device memory, given as float64 tensors or device addresses; both
    None (the default) turns it off.  One without the other is refused."""
    x, y = _device_address(jx), _device_address(jy)
    if (x is None) != (y is None):
        raise ValueError("the current is kept as both of Jx and Jy or neither")
    if _lib.neutral_hip_set_current_tally(x, y) != 0:
        raise ValueError("the current is kept as both of Jx and Jy or neither")


def set_outflow_tally(buf=None) -> None:
    """The outflow tally of the following steps (include/neutral_hip.h): the weight that leaves
    each cell through its west, east, south and north side, four meshes of ny*nx doubles back to
    back in one buffer of device memory, given as a float64 tensor or a device address; None or a
    null address (the default) turns it off."""
    address = _device_address(buf)
    if address is None and not hasattr(_lib, "neutral_hip_set_outflow_tally"):
        return   # (an older build: nothing to turn off)
    _lib.neutral_hip_set_outflow_tally(address)


VACUUM_SIDES = {"w": 1 << 0, "e": 1 << 1, "s": 1 << 2, "n": 1 << 3}  # (the outflow tally's side numbers)
VACUUM_SIDE_NAMES = ("west", "east", "south", "north")


def vacuum_mask(sides) -> int:
    """The mask neutral_hip_set_vacuum_sides takes, from the letters w e s n in any case and any
    order ("wn" -> 9), "all", "" or None (0: every wall reflects), or an int 0..15 as it is.  Raises
    ValueError on anything else.  Needs no GPU."""
    if sides is None:
        return 0
    if isinstance(sides, bool):
        raise ValueError(f"vacuum sides {sides!r}: letters of 'wesn', 'all', or a mask 0..15")
    if isinstance(sides, (int, np.integer)):
        if not 0 <= int(sides) <= 15:
            raise ValueError(f"vacuum sides {sides!r}: a mask has the bits 1 (west), 2 (east), 4 (south), 8 (north)")
        return int(sides)
    if not isinstance(sides, str):
        raise ValueError(f"vacuum sides {sides!r}: letters of 'wesn', 'all', or a mask 0..15")
    text = sides.strip().lower()
    if text == "all":
        return 15
    mask = 0
    for letter in text:
        if letter not in VACUUM_SIDES:
            raise ValueError(f"vacuum sides {sides!r}: letters of 'wesn', 'all', or a mask 0..15")
        mask |= VACUUM_SIDES[letter]
    return mask


def set_vacuum_sides(sides=0) -> None:
    """The outer sides histories escape through in the following steps (include/neutral_hip.h:
    neutral_hip_set_vacuum_sides), as vacuum_mask() reads them; 0, the default: every wall
    reflects.  Raises ValueError, and changes nothing, on a bit above 8."""
    mask = sides if isinstance(sides, (int, np.integer)) and not isinstance(sides, bool) else vacuum_mask(sides)
    if not 0 <= int(mask) < 2 ** 32 or _lib.neutral_hip_set_vacuum_sides(int(mask)) != 0:
        raise ValueError(f"vacuum sides {sides!r} refused: a mask has the bits 1 (west), 2 (east), 4 (south), 8 (north)")


def get_vacuum_sides() -> int:
    return int(_lib.neutral_hip_get_vacuum_sides())


def last_escape() -> EscapeStats:
    """The last step's escapes by side and the sum of their weights, over the ranks
    (neutral_hip_last_escape); all zero when no side is vacuum."""
    stats = EscapeStats()
    if hasattr(_lib, "neutral_hip_last_escape"):   # (an older build has no vacuum sides: zeros)
        _lib.neutral_hip_last_escape(C.byref(stats))
    return stats


PERIODIC_AXES = {"x": 1 << 0, "y": 1 << 1}  # (x: west <-> east; y: south <-> north)


def periodic_mask(axes) -> int:
    """The mask neutral_hip_set_periodic_axes takes, from the letters x y in any case and any order
    ("xy" -> 3), "" or None (0: no axis is periodic), or an int 0..3 as it is.  Raises ValueError on
    anything else.  Needs no GPU."""
    if axes is None:
        return 0
    if isinstance(axes, bool):
        raise ValueError(f"periodic axes {axes!r}: letters of 'xy', or a mask 0..3")
    if isinstance(axes, (int, np.integer)):
        if not 0 <= int(axes) <= 3:
            raise ValueError(f"periodic axes {axes!r}: a mask has the bits 1 (x) and 2 (y)")
        return int(axes)
    if not isinstance(axes, str):
        raise ValueError(f"periodic axes {axes!r}: letters of 'xy', or a mask 0..3")
    mask = 0
    for letter in axes.strip().lower():
        if letter not in PERIODIC_AXES:
            raise ValueError(f"periodic axes {axes!r}: letters of 'xy', or a mask 0..3")
        mask |= PERIODIC_AXES[letter]
    return mask


def periodic_sides(axes: int) -> int:
    """the outer sides of the axes in a periodic mask, as a vacuum mask (x: west and east; y: south
    and north)"""
    return (3 if axes & 1 else 0) | (12 if axes & 2 else 0)


def set_periodic_axes(axes=0) -> None:
    """The axes whose outer sides are one seam in the following steps (include/neutral_hip.h:
    neutral_hip_set_periodic_axes), as periodic_mask() reads them; 0, the default: none.  Raises
    ValueError, and changes nothing, on a bit above 2 or while a side of a requested axis is vacuum."""
    mask = axes if isinstance(axes, (int, np.integer)) and not isinstance(axes, bool) else periodic_mask(axes)
    if not 0 <= int(mask) < 2 ** 32 or _lib.neutral_hip_set_periodic_axes(int(mask)) != 0:
        raise ValueError(f"periodic axes {axes!r} refused: a mask has the bits 1 (x) and 2 (y), and no side of "
                         "a periodic axis may be vacuum")


def get_periodic_axes() -> int:
    return int(_lib.neutral_hip_get_periodic_axes())


def last_wraps() -> WrapStats:
    """The last step's wraps by the side left through and the sum of their weights, over the ranks
    (neutral_hip_last_wraps); all zero when no axis is periodic."""
    stats = WrapStats()
    if hasattr(_lib, "neutral_hip_last_wraps"):   # (an older build has no periodic axes: zeros)
        _lib.neutral_hip_last_wraps(C.byref(stats))
    return stats


_roulette = (0.0, 0.0)  # what set_roulette last set in the library (process-global)


def set_roulette(weight_cutoff: float = 0.0, survival_weight: float = 0.0) -> None:
    """Weight cutoff with Russian roulette for the following steps (include/neutral_hip.h):
    an absorption that leaves a weight w below weight_cutoff keeps the history with weight
    survival_weight at probability w / survival_weight and ends it otherwise.  (0, 0), the
    default, turns it off.  Raises ValueError, and changes nothing, where the library refuses:
    a NaN, infinite or negative value, exactly one of them 0, survival_weight < weight_cutoff."""
    global _roulette
    wc, ws = float(weight_cutoff), float(survival_weight)
    if _lib.neutral_hip_set_roulette(wc, ws) != 0:
        raise ValueError(f"roulette ({weight_cutoff}, {survival_weight}) refused: both 0 (off), or "
                         "finite with 0 < weight_cutoff <= survival_weight")
    _roulette = (wc, ws)


def set_window_roulette(nx: int, ny: int, lower, survival_ratio: float = 3.0, groups=None, block=None) -> None:
    """The in-step weight window for the following steps (include/neutral_hip.h:
    neutral_hip_set_window_roulette): roulette inside the steps with the cutoff taken per bin from
    `lower`, the census window's mesh of lower bounds for the GLOBAL mesh of nx by ny -- a float64
    device tensor or a device address of max(G, 1) * cny * cnx values, which must stay allocated
    while set and may be rewritten between steps.  None (or a null address) turns it off; the
    other arguments are ignored then.  groups: the G + 1 edges of energy groups; block: (block_x,
    block_y) or one int.  Raises ValueError, and changes nothing, where the library refuses: a
    size < 1, a survival_ratio not finite or < 1, invalid groups or blocks, a mesh entry that is
    negative or not finite, or a global cutoff (set_roulette) in force."""
    address = _device_address(lower)
    if not hasattr(_lib, "neutral_hip_set_window_roulette"):
        if address is None:
            return   # (an older build: nothing to turn off)
        raise RuntimeError("this build of the library has no in-step weight window")
    if address is None:
        _lib.neutral_hip_set_window_roulette(0, 0, None, 0.0, 0, None, 1, 1)
        return
    _checked(("mesh width", nx, _INT32, f"nx {nx} is not an int32"),
             ("mesh height", ny, _INT32, f"ny {ny} is not an int32"))
    try:
        e = None if groups is None else np.ascontiguousarray(groups, dtype=np.float64).ravel()
    except (TypeError, ValueError):
        raise ValueError(f"energy group edges {groups!r} are not numbers") from None
    if e is not None and not 2 <= e.size <= GROUPS_MAX + 1:
        raise ValueError(f"energy groups need 2 to {GROUPS_MAX + 1} edges, not {e.size}")
    pair = (1, 1) if block is None else (tuple(block) if isinstance(block, (tuple, list, np.ndarray)) else (block, block))
    if len(pair) != 2:
        raise ValueError(f"a block is one int or (block_x, block_y), not {block!r}")
    _checked(("block width", pair[0], _INT32, f"block {block!r} is not of int32s"),
             ("block height", pair[1], _INT32, f"block {block!r} is not of int32s"))
    code = _lib.neutral_hip_set_window_roulette(
        int(nx), int(ny), address, float(survival_ratio), 0 if e is None else e.size - 1,
        None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)), int(pair[0]), int(pair[1]))
    if code != 0:
        raise ValueError(f"in-step window refused (nx {nx}, ny {ny}, survival_ratio {survival_ratio}, groups "
                         f"{groups!r}, block {block!r}): sizes and blocks >= 1, a finite ratio >= 1, valid "
                         "edges, no mesh entry negative or not finite, no global cutoff set")


COMB_TILE = 2048  # elements per workgroup of the comb's scans (neutral_kernels.h: kCombTile)
_INT32, _UINT64 = (-2 ** 31, 2 ** 31), (0, 2 ** 64)
_COUNT = (0, 2 ** 31)       # ... of particles to emit: none is a count
_POSITIVE = (1, 2 ** 31)    # ... of what there has to be some of: slots of a store, cells of a mesh


def _checked(*integers, particles=True):
    """The arguments every call between two steps checks before the library sees them: `particles`,
    the store (a call without one names none), and integers as (name, value, (lo, hi), message).
    TypeError for a value that is not an integer (a bool is none), then ValueError(message) for one
    outside lo <= value < hi, each in the order given."""
    if not particles:
        raise ValueError("no particle store")
    for name, v, _, _ in integers:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"a {name} is an integer, not {type(v).__name__}")
    for _, v, (lo, hi), message in integers:
        if not lo <= int(v) < hi:
            raise ValueError(message)


def _emission(n, count, seed):
    """what the three sources take: the store's size, how many to emit, the master key"""
    return (("particle count", n, _POSITIVE, f"no store holds {n} particles"),
            ("count", count, _COUNT, f"cannot emit {count} particles"),
            ("seed", seed, _UINT64, f"seed {seed} is not a uint64"))


class Refused(ValueError):
    """What the *Refused below share: `code`, the library's return code, which picks the message,
    and `stats`, what the library had filled in by then."""
    code_1 = otherwise = ""

    def __init__(self, code, stats):
        super().__init__(self.code_1 if code == 1 else self.otherwise)
        self.code, self.stats = code, stats


class CombRefused(Refused):
    """The library left the store as it was: code 1 -- nothing live, a total weight that is not
    positive and finite, or a live weight that is negative or not finite; code 2 -- a decomposed
    store.  `stats` holds what the scan found (code 1)."""
    code_1 = "nothing to comb: no live particle, or a live weight that is negative or not finite"
    otherwise = "a decomposed store cannot be combed"


def comb_particles(particles, n: int, seed: int) -> CombStats:
    """The census weight comb (include/neutral_hip.h: neutral_hip_comb_particles) on a store of n
    particles, between two steps: resamples the live particles to n equal weights, refills every
    dead slot.  The offset comes from `seed` and the pid base in force (set_pid_base).  Raises
    CombRefused, a ValueError, where the library changes nothing."""
    _checked(("particle count", n, _POSITIVE, f"cannot comb {n} particles"),
             ("seed", seed, _UINT64, f"seed {seed} is not a uint64"), particles=particles)
    stats = CombStats()
    code = _lib.neutral_hip_comb_particles(particles, int(n), int(seed), C.byref(stats))
    if code != 0:
        raise CombRefused(code, stats)
    return stats


SOURCE_SEED_BASE = 2 ** 63  # emit's and the driver's seeds: 2^63 + tt, which no timestep number is


class SourceRefused(Refused):
    """The library left the store as it was: code 1 -- a count below 0, a weight, energy or dt that
    is not finite and positive, a box whose width or height is negative or not finite, no mesh;
    code 2 -- a decomposed store."""
    code_1 = ("source refused: count >= 0, weight, energy and dt finite and positive, a box "
              "of finite non-negative width and height")
    otherwise = "a decomposed store takes no source"


def source_particles(particles, n: int, count: int, weight: float, seed: int, local_nx, local_ny,
                     pad, left_off, bottom_off, width, height, x_off, y_off, dt, edgex, edgey,
                     initial_energy) -> SourceStats:
    """The fixed source (include/neutral_hip.h: neutral_hip_source_particles) on a store of n
    particles, between two steps: the first `count` dead slots, in index order, become fresh source
    particles of `weight` drawn with master key `seed`; the arguments from local_nx on are
    injection's.  The particle keys come from the pid base in force (set_pid_base).  Raises
    SourceRefused, a ValueError, where the library changes nothing."""
    _checked(*_emission(n, count, seed), particles=particles)
    stats = SourceStats()
    code = _lib.neutral_hip_source_particles(
        particles, int(n), int(count), float(weight), int(seed), local_nx, local_ny, pad,
        float(left_off), float(bottom_off), float(width), float(height), x_off, y_off, float(dt),
        edgex, edgey, float(initial_energy), C.byref(stats))
    if code != 0:
        raise SourceRefused(code, stats)
    return stats


class SourceComponent:
    """One component of a described source: a relative emission rate, a box (left, bottom, width,
    height), a spectrum and an interval of the direction angle, theta = (theta0, theta_width).
    `energies` lists (e, share) lines and (e_lo, e_hi, share) bins, uniform in energy."""

    def __init__(self, share, box, energies, theta=(0.0, 2.0 * np.pi)):
        self.share = float(share)
        self.box = tuple(float(v) for v in box)
        if len(self.box) != 4:
            raise ValueError("a box is (left, bottom, width, height)")
        self.theta = tuple(float(v) for v in theta)
        if len(self.theta) != 2:
            raise ValueError("theta is (theta0, theta_width)")
        self.bins = []
        for e in energies:
            e = tuple(float(v) for v in e)
            if len(e) not in (2, 3):
                raise ValueError("an energy is a line (e, share) or a bin (e_lo, e_hi, share)")
            self.bins.append((e[0], e[0], e[1]) if len(e) == 2 else e)
        if not self.bins:
            raise ValueError("a component needs at least one energy")


class DescribedSourceRefused(Refused):
    """The library left the store as it was: code 1 -- what SourceRefused names, or a description
    it does not take (a share that is not finite and positive, a box, angle or energy interval
    that is not finite or runs backwards, a bin range outside the table); code 2 -- a decomposed
    store."""
    code_1 = ("described source refused: count >= 0, weight and dt finite and positive, "
              "shares finite and positive, boxes, angle and energy intervals finite and "
              "not backwards, energies positive")
    otherwise = "a decomposed store takes no source"


class SourceDescription:
    """A described source (include/neutral_hip.h: neutral_hip_source_described): its components,
    flattened to the library's two tables, every component's bins in order behind the last one's."""
    refused, stats = DescribedSourceRefused, DescribedSourceStats  # (what Simulation raises for it)
    no_box = "a described source has its own energies and boxes"  # (emit's, for energy= or box=)

    def emit(self, particles, n, count, weight, seed, device, *mesh):
        """source_described out of this description; mesh: its arguments from local_nx on"""
        return source_described(particles, n, count, weight, seed, self, *mesh)

    def __init__(self, components):
        self.components = list(components)
        if not 1 <= len(self.components) <= SOURCE_MAX_COMPONENTS:
            raise ValueError(f"a description has 1 to {SOURCE_MAX_COMPONENTS} components")
        nbins = sum(len(c.bins) for c in self.components)
        if nbins > SOURCE_MAX_BINS:
            raise ValueError(f"a description has at most {SOURCE_MAX_BINS} lines and bins")
        self.component_table = (SourceComponentC * len(self.components))()
        self.bin_table = (SourceBinC * nbins)()
        first = 0
        for k, c in enumerate(self.components):
            self.component_table[k] = SourceComponentC(c.share, *c.box, *c.theta, first, len(c.bins))
            for b, (e_lo, e_hi, share) in enumerate(c.bins):
                self.bin_table[first + b] = SourceBinC(e_lo, e_hi, share)
            first += len(c.bins)

    def check(self, problem, cs_keys):
        """ValueError for what the library does not look at: a box that leaves the mesh, an energy
        outside [max(1.0, keys.min()), keys.max()] of the cross-section tables"""
        keys = np.asarray(cs_keys, dtype=np.float64)
        e_min, e_max = max(1.0, float(keys.min())), float(keys.max())
        x0, x1 = float(problem.edgex[problem.pad]), float(problem.edgex[problem.pad + problem.nx])
        y0, y1 = float(problem.edgey[problem.pad]), float(problem.edgey[problem.pad + problem.ny])
        for k, c in enumerate(self.components):
            left, bottom, width, height = c.box
            if not (width >= 0.0 and height >= 0.0 and x0 <= left and left + width <= x1
                    and y0 <= bottom and bottom + height <= y1):
                raise ValueError(f"component {k}: box {c.box} leaves the mesh "
                                 f"[{x0}, {x1}] x [{y0}, {y1}]")
            for e_lo, e_hi, _ in c.bins:
                if not e_min <= e_lo <= e_hi <= e_max:
                    raise ValueError(f"component {k}: energies [{e_lo}, {e_hi}] leave the cross-section "
                                     f"tables' [{e_min}, {e_max}]")


def source_described(particles, n: int, count: int, weight: float, seed: int,
                     description: SourceDescription, local_nx, local_ny, pad, x_off, y_off, dt,
                     edgex, edgey) -> DescribedSourceStats:
    """The described source (include/neutral_hip.h: neutral_hip_source_described) on a store of n
    particles, between two steps: the first `count` dead slots, in index order, become particles of
    `weight` out of `description`, drawn with master key `seed`.  The particle keys come from the
    pid base in force (set_pid_base).  Raises DescribedSourceRefused, a ValueError, where the
    library changes nothing."""
    if particles and not isinstance(description, SourceDescription):
        raise TypeError(f"a description is a SourceDescription, not {type(description).__name__}")
    _checked(*_emission(n, count, seed), particles=particles)
    stats = DescribedSourceStats()
    code = _lib.neutral_hip_source_described(
        particles, int(n), int(count), float(weight), int(seed),
        len(description.component_table), description.component_table,
        len(description.bin_table), description.bin_table,
        local_nx, local_ny, pad, x_off, y_off, float(dt), edgex, edgey, C.byref(stats))
    if code != 0:
        raise DescribedSourceRefused(code, stats)
    return stats


ISOTROPIC = (0.0, 2.0 * np.pi)  # theta of a source that emits in every direction, as injection does


class MeshSourceRefused(Refused):
    """The library left the store as it was: code 1 -- what SourceRefused names, an angle interval
    or a spectrum the described source would not take, or, found on the device, a strength that is
    negative or not finite or a mesh without any; code 2 -- a decomposed store."""
    code_1 = ("mesh source refused: count >= 0, weight and dt finite and positive, strengths "
              "finite and not negative with one above zero, shares finite and positive, angle "
              "and energy intervals finite and not backwards, energies positive")
    otherwise = "a decomposed store takes no source"


class MeshSource:
    """A mesh source (include/neutral_hip.h: neutral_hip_source_mesh): particles are born in cell
    (j, i) in proportion to strength[j, i], uniformly inside it.  `strength` is a float64 device
    tensor of ny * nx values, used in place (one of a Simulation's own tallies, say: every call
    reads what it holds then), or a numpy array of shape (ny, nx), copied here and uploaded once
    to every device the source is used on (later changes to the caller's array do not show).
    `energies` lists (e, share)
    lines and (e_lo, e_hi, share) bins as SourceComponent takes them: one spectrum for every cell;
    theta = (theta0, theta_width) is the interval of the direction angle."""
    refused, stats = MeshSourceRefused, MeshSourceStats  # (what Simulation raises for it)
    no_box = "a mesh source has its own energies and cells"  # (emit's, for energy= or box=)

    def emit(self, particles, n, count, weight, seed, device, *mesh):
        """source_mesh out of this mesh, on `device`; mesh: its arguments from local_nx on"""
        return source_mesh(particles, n, count, weight, seed, self.device_pointer(device), self.theta,
                           self.bin_table, *mesh)

    def __init__(self, strength, energies, theta=ISOTROPIC):
        one = SourceComponent(1.0, (0.0, 0.0, 0.0, 0.0), energies, theta)  # (its parsing, its errors)
        self.bins, self.theta = one.bins, one.theta
        if len(self.bins) > SOURCE_MAX_BINS:
            raise ValueError(f"a spectrum has at most {SOURCE_MAX_BINS} lines and bins")
        self.bin_table = (SourceBinC * len(self.bins))(*(SourceBinC(*b) for b in self.bins))
        self.on_device = isinstance(strength, torch.Tensor)
        if self.on_device:
            if strength.dtype != torch.float64 or not strength.is_cuda or not strength.is_contiguous():
                raise ValueError("a strength tensor is a contiguous float64 tensor on the device")
            self.strength, self.shape = strength, tuple(strength.shape)
        else:
            self.strength = np.array(strength, dtype=np.float64, order="C")  # (a copy: see above)
            self.shape = self.strength.shape
            self._uploaded = {}  # by device

    def check(self, problem, cs_keys):
        """ValueError for what the library does not look at or finds late: a strength that is not
        the problem's mesh ((ny, nx); a device tensor may be flat), an energy outside
        [max(1.0, keys.min()), keys.max()] of the cross-section tables, and in a numpy array an
        entry that is negative or not finite"""
        nx, ny = problem.nx, problem.ny
        if self.shape != (ny, nx) and not (self.on_device and self.shape == (ny * nx,)):
            raise ValueError(f"strength has shape {self.shape}: the mesh is {ny} x {nx}")
        keys = np.asarray(cs_keys, dtype=np.float64)
        e_min, e_max = max(1.0, float(keys.min())), float(keys.max())
        for e_lo, e_hi, _ in self.bins:
            if not e_min <= e_lo <= e_hi <= e_max:
                raise ValueError(f"energies [{e_lo}, {e_hi}] leave the cross-section tables' [{e_min}, {e_max}]")
        if not self.on_device and not (np.all(np.isfinite(self.strength)) and np.all(self.strength >= 0.0)):
            raise ValueError("a strength is negative or not finite")

    def device_pointer(self, device="cuda") -> int:
        """the strengths on `device`: a device tensor's own pointer (it must live there), a numpy
        array's upload to that device, made once"""
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if self.on_device:
            if self.strength.device != device:
                raise ValueError(f"the strength tensor lives on {self.strength.device}, the store on {device}")
            return self.strength.data_ptr()
        if device not in self._uploaded:
            self._uploaded[device] = torch.from_numpy(self.strength).to(device)
        return self._uploaded[device].data_ptr()


def source_mesh(particles, n: int, count: int, weight: float, seed: int, strength, theta, bin_table,
                local_nx, local_ny, pad, x_off, y_off, dt, edgex, edgey) -> MeshSourceStats:
    """The mesh source (include/neutral_hip.h: neutral_hip_source_mesh) on a store of n particles,
    between two steps: the first `count` dead slots, in index order, become particles of `weight` born
    in proportion to `strength`, a device pointer to local_ny rows of local_nx doubles, with the
    spectrum `bin_table` (a ctypes array of SourceBinC) and the angle interval theta = (theta0,
    theta_width), drawn with master key `seed`.  The particle keys come from the pid base in force
    (set_pid_base).  Raises MeshSourceRefused, a ValueError, where the library changes nothing."""
    if not hasattr(_lib, "neutral_hip_source_mesh"):
        raise RuntimeError("this build of the library has no mesh source")
    _checked(*_emission(n, count, seed), particles=particles)
    if isinstance(strength, bool) or not (strength is None or isinstance(strength, (int, np.integer))):
        raise TypeError(f"a strength is a device pointer, not {type(strength).__name__}")
    if bin_table is not None and not (isinstance(bin_table, C.Array) and bin_table._type_ is SourceBinC):
        raise TypeError(f"a bin table is an array of SourceBinC, not {type(bin_table).__name__}")
    theta0, theta_width = theta
    stats = MeshSourceStats()
    code = _lib.neutral_hip_source_mesh(
        particles, int(n), int(count), float(weight), int(seed),
        C.c_void_p(int(strength)) if strength else None, float(theta0), float(theta_width),
        len(bin_table) if bin_table is not None else 0, bin_table,
        local_nx, local_ny, pad, x_off, y_off, float(dt), edgex, edgey, C.byref(stats))
    if code != 0:
        raise MeshSourceRefused(code, stats)
    return stats


_escape_bank = None  # (address, capacity) of the bank the library was last given; None: off


def set_escape_bank(records=None, capacity: int = 0) -> None:
    """The escape bank for the following steps (include/neutral_hip.h): every history that escapes
    through a vacuum side is appended to `records`, a device tensor (or address) with room for
    `capacity` records of 64 bytes, 16-byte aligned.  records=None turns it off.  A successful call
    starts the bank at index 0.  Raises ValueError, and changes nothing, where the library refuses:
    capacity 0, a pointer that is not 16-byte aligned."""
    global _escape_bank
    if records is None:
        _lib.neutral_hip_set_escape_bank(None, 0)
        _escape_bank = None
        return
    _checked(("capacity", capacity, _UINT64, f"capacity {capacity} is not a uint64"))
    if hasattr(records, "numel") and records.numel() * records.element_size() < 64 * int(capacity):
        raise ValueError(f"the tensor holds {records.numel() * records.element_size()} bytes, {capacity} records "
                         f"need {64 * int(capacity)}")
    if hasattr(records, "data_ptr"):
        if not records.is_contiguous():
            raise ValueError("a bank tensor must be contiguous")
        ptr = records.data_ptr()
    elif isinstance(records, (int, np.integer)) and not isinstance(records, bool):
        ptr = int(records)
    else:
        raise TypeError(f"not a device array: {type(records).__name__}")
    if _lib.neutral_hip_set_escape_bank(C.c_void_p(ptr), int(capacity)) != 0:
        raise ValueError(f"escape bank refused (address {ptr:#x}, capacity {capacity}): a capacity of at least "
                         "1, records 16-byte aligned")
    _escape_bank = (ptr, int(capacity))


def reset_escape_bank() -> None:
    """The bank's cursor back to 0; the records stay as they are.  RuntimeError while the bank is off."""
    if _lib.neutral_hip_reset_escape_bank() != 0:
        raise RuntimeError("no escape bank is set")


def escape_bank_stats() -> EscapeBankStats:
    """The bank's capacity and cursor, what it holds, and the last step's claimed and recorded."""
    stats = EscapeBankStats()
    _lib.neutral_hip_escape_bank_stats(C.byref(stats))
    return stats


class BankSourceRefused(Refused):
    """The library left the store as it was: code 1 -- what SourceRefused names, a weight scale that
    is not finite and positive, a snap distance that is negative or not finite, a shift that is not
    finite; code 2 -- a decomposed store; code 3 -- found on the device before anything is written:
    a record with a side above 3, a field that is not finite, a weight or an energy that is not
    positive, both cosines zero, or a shifted position outside the mesh by more than the snap
    distance.  `first_bad` is the lowest index of such a record (None otherwise)."""
    code_1 = ("bank source refused: count >= 0, weight scale and dt finite and positive, a finite "
              "snap distance >= 0, finite shifts")
    otherwise = "a decomposed store takes no source"

    def __init__(self, code, stats):
        super().__init__(code, stats)
        self.first_bad = int(stats.first_bad) if code == 3 else None
        if code == 3:
            self.args = (f"bank source refused: record {self.first_bad} has a side above 3, a field that is not "
                         "finite, a weight or energy that is not positive, no direction, or lies outside the "
                         "mesh by more than the snap distance",)


NO_SHIFT = (0.0,) * 8


def periodic_shift(width: float, height: float):
    """the shift that makes a periodic boundary of vacuum sides: what leaves west re-enters at the
    east wall, east at the west wall, south at the north wall, north at the south wall"""
    return (float(width), 0.0, -float(width), 0.0, 0.0, float(height), 0.0, -float(height))


def source_bank(particles, n: int, records, first: int, count: int, weight_scale: float, shift, snap: float,
                local_nx, local_ny, pad, x_off, y_off, dt, edgex, edgey) -> BankSourceStats:
    """The bank source (include/neutral_hip.h: neutral_hip_source_bank) on a store of n particles,
    between two steps: the first `count` dead slots, in index order, take the escape records
    records[first], records[first + 1], ... (`records`: a device address), each moved by
    shift[2 * side], shift[2 * side + 1] (eight values; None: zeros), snapped onto a wall it misses by
    at most `snap`, at its weight times weight_scale.  Nothing is drawn.  Raises BankSourceRefused, a
    ValueError, where the library changes nothing."""
    _checked(("particle count", n, _POSITIVE, f"no store holds {n} particles"),
             ("count", count, _COUNT, f"cannot emit {count} particles"),
             ("first", first, _UINT64, f"first {first} is not a uint64"), particles=particles)
    if isinstance(records, bool) or not (records is None or isinstance(records, (int, np.integer))):
        raise TypeError(f"records is a device pointer, not {type(records).__name__}")
    s = None
    if shift is not None:
        values = [float(v) for v in shift]
        if len(values) != 8:
            raise ValueError(f"a shift is (dx, dy) for the four sides, eight values, not {len(values)}")
        s = (C.c_double * 8)(*values)
    stats = BankSourceStats()
    code = _lib.neutral_hip_source_bank(
        particles, int(n), C.c_void_p(int(records)) if records else None, int(first), int(count),
        float(weight_scale), s, float(snap), local_nx, local_ny, pad, x_off, y_off, float(dt), edgex, edgey,
        C.byref(stats))
    if code != 0:
        raise BankSourceRefused(code, stats)
    return stats


class BankSource:
    """A bank source (include/neutral_hip.h: neutral_hip_source_bank): dead slots are refilled from
    escape records instead of being sampled.  `records` is a uint8 device tensor of 64-byte records,
    used in place (a Simulation's own bank, say: every call reads what it holds then), or a numpy
    structured array of ESCAPE_RECORD, copied here and uploaded once to every device the source is
    used on.  Slot d_k of the dead slots takes record first + k.  shift: (dx, dy) for each side a
    record left through, eight values (periodic_shift); snap: how far outside a wall a shifted
    position may lie and be put on it.  emit()'s weight multiplies weight_scale; its seed is not
    used: nothing is drawn."""
    refused, stats = BankSourceRefused, BankSourceStats  # (what Simulation raises for it)
    no_box = "a bank source has its records' energies and positions"  # (emit's, for energy= or box=)

    def __init__(self, records, first: int = 0, shift=None, weight_scale: float = 1.0, snap: float = 0.0):
        self.on_device = isinstance(records, torch.Tensor)
        if self.on_device:
            if records.dtype != torch.uint8 or not records.is_cuda or not records.is_contiguous() or \
                    records.numel() % 64 != 0:
                raise ValueError("a bank tensor is a contiguous uint8 tensor of 64-byte records on the device")
            self.records, self.count = records, records.numel() // 64
        else:
            self.records = np.array(records, dtype=ESCAPE_RECORD, order="C").ravel()  # (a copy)
            self.count = len(self.records)
            self._uploaded = {}  # by device
        self.first, self.weight_scale, self.snap = int(first), float(weight_scale), float(snap)
        self.shift = None if shift is None else tuple(float(v) for v in shift)
        if self.shift is not None and len(self.shift) != 8:
            raise ValueError(f"a shift is (dx, dy) for the four sides, eight values, not {len(self.shift)}")

    def check(self, problem, cs_keys):
        """ValueError for what the library cannot know: a first record past the end of the bank"""
        if not 0 <= self.first <= self.count:
            raise ValueError(f"first {self.first}: the bank holds {self.count} records")

    def device_pointer(self, device="cuda") -> int:
        """the records on `device`: a device tensor's own pointer (it must live there), a numpy
        array's upload to that device, made once"""
        device = torch.device(device)
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if self.on_device:
            if self.records.device != device:
                raise ValueError(f"the bank tensor lives on {self.records.device}, the store on {device}")
            return self.records.data_ptr()
        if device not in self._uploaded:
            host = torch.from_numpy(self.records.view(np.uint8).copy())
            self._uploaded[device] = host.to(device) if len(host) else torch.zeros(64, dtype=torch.uint8, device=device)
        return self._uploaded[device].data_ptr()

    def emit(self, particles, n, count, weight, seed, device, *mesh):
        """source_bank out of these records, on `device`; mesh: its arguments from local_nx on.  At
        most the records from `first` on are used, however many slots are dead."""
        count = min(int(count), self.count - self.first)
        return source_bank(particles, n, self.device_pointer(device), self.first, count,
                           self.weight_scale * float(weight), self.shift, self.snap, *mesh)


WINDOW_SEED_BASE = 2 ** 63 + 2 ** 62  # window's and the driver's seeds: this + tt, which no timestep,
#                                       injection (0) or source (2^63 + tt) uses


class WindowRefused(Refused):
    """The library left the store as it was: code 1 -- no mesh of bounds, ratios that are not finite,
    upper_ratio < 2, survival_ratio outside [1, upper_ratio], max_split outside 2..64, or a live slot
    with a cell outside the mesh, a weight or a bound that is negative or not finite; code 2 -- a
    decomposed store."""
    code_1 = ("window refused: upper_ratio >= 2, 1 <= survival_ratio <= upper_ratio, "
              "2 <= max_split <= 64, live cells inside the mesh, weights and bounds finite "
              "and not negative")
    otherwise = "a decomposed store takes no window"


def window_particles(particles, n: int, nx: int, ny: int, lower, upper_ratio: float,
                     survival_ratio: float, max_split: int, seed: int) -> WindowStats:
    """The census weight window (include/neutral_hip.h: neutral_hip_window_particles) on a store of n
    particles, between two steps: a live history under lower[cell] plays roulette for survival_ratio
    times the bound, one over upper_ratio times the bound is split into at most max_split, the copies
    going to free slots in index order.  `lower` is a device pointer to ny * nx doubles.  The
    particle keys come from the pid base in force (set_pid_base).  Raises WindowRefused, a
    ValueError, where the library changes nothing."""
    _checked(("particle count", n, _POSITIVE, f"no store holds {n} particles"),
             ("mesh width", nx, _POSITIVE, f"no mesh of {nx} x {ny} cells"),
             ("mesh height", ny, _POSITIVE, f"no mesh of {nx} x {ny} cells"),
             ("split limit", max_split, _INT32, f"max_split {max_split} is not an int"),
             ("seed", seed, _UINT64, f"seed {seed} is not a uint64"), particles=particles)
    stats = WindowStats()
    code = _lib.neutral_hip_window_particles(
        particles, int(n), int(nx), int(ny), lower, float(upper_ratio), float(survival_ratio),
        int(max_split), int(seed), C.byref(stats))
    if code != 0:
        raise WindowRefused(code, stats)
    return stats


class CensusRefused(Refused):
    """The library tallied nothing: code 1 -- no store or no mesh, or a live slot with a cell outside
    the mesh or a weight that is negative or not finite; code 2 -- a decomposed store."""
    code_1 = "census refused: live cells inside the mesh, weights finite and not negative"
    otherwise = "a decomposed store takes no census"


def _mesh_size(nx, ny):
    _checked(("mesh width", nx, _POSITIVE, f"no mesh of {nx} x {ny} cells"),
             ("mesh height", ny, _POSITIVE, f"no mesh of {nx} x {ny} cells"))
    if not int(nx) * int(ny) < 2 ** 30:
        raise ValueError(f"no mesh of {nx} x {ny} cells")
    return int(nx), int(ny)


def census_tally(particles, n: int, nx: int, ny: int, out=None):
    """The census tally (include/neutral_hip.h: neutral_hip_census_tally) of a store of n particles,
    between two steps: -> (count, weight, stats), two float64 device tensors of ny * nx values --
    the live histories per cell and the weight they carry -- and CensusStats.  A snapshot: the
    meshes are zeroed first.  out: a float64 device tensor of 2 * ny * nx values to tally into (the
    two results are its halves); None: a new one.  The store is not written to.  Raises
    CensusRefused, a ValueError, where the library tallies nothing."""
    _checked(("particle count", n, _COUNT, f"no store holds {n} particles"), particles=particles)
    # (the call is collective: a rank whose shard of a sharded store is empty -- fewer particles than
    # ranks -- makes it like the others, with zeros, or they would wait for it)
    empty_shard = int(n) == 0 and _lib.neutral_hip_comm_nranks() > 1 and _lib.neutral_hip_store_count(particles) == 0
    if int(n) == 0 and not empty_shard:
        raise ValueError(f"no store holds {n} particles")
    nx, ny = _mesh_size(nx, ny)
    if out is None:
        out = torch.empty(2 * nx * ny, dtype=torch.float64, device="cuda")
    elif out.dtype != torch.float64 or out.numel() != 2 * nx * ny or not out.is_contiguous():
        raise ValueError(f"out holds {out.numel()} {out.dtype} values: the census needs 2 * {ny} * {nx} float64")
    stats = CensusStats()
    code = _lib.neutral_hip_census_tally(particles, int(n), nx, ny, C.c_void_p(out.data_ptr()),
                                         C.byref(stats))
    if code != 0:
        raise CensusRefused(code, stats)
    return out[:nx * ny], out[nx * ny:], stats


class BoundsRefused(Refused):
    """The library made no bounds: code 1 -- a target_population that is not finite and positive,
    upper_ratio < 2 or not finite, floor_ratio outside [0, 1], min_count < 1, a census entry that
    is negative or not finite, or no eligible cell."""
    code_1 = otherwise = ("bounds refused: target_population > 0, upper_ratio >= 2, 0 <= floor_ratio <= 1, "
                          "min_count >= 1, a census of finite entries that are not negative and at "
                          "least one eligible cell")


def window_bounds(nx: int, ny: int, census, target_population: float, upper_ratio: float = 5.0,
                  floor_ratio: float = 0.0, min_count: int = 1, out=None):
    """Lower bounds for the census weight window from a census tally (include/neutral_hip.h:
    neutral_hip_window_bounds): -> (lower, stats), a float64 device tensor of ny * nx bounds,
    proportional to the cells' weight and scaled so that the eligible cells together settle at
    target_population histories, and BoundsStats.  census: a float64 device tensor of 2 * ny * nx
    values, counts then weights, as census_tally fills its `out`.  out: the tensor to write the
    bounds to; None: a new one.  Raises BoundsRefused, a ValueError, where the library makes none
    (out is then untouched)."""
    nx, ny = _mesh_size(nx, ny)
    _checked(("count", min_count, _INT32, f"min_count {min_count} is not an int"))
    if not hasattr(census, "data_ptr") or census.dtype != torch.float64 or census.numel() != 2 * nx * ny \
            or not census.is_contiguous():
        raise ValueError(f"the census of a {ny} x {nx} mesh is a float64 device tensor of 2 * {ny} * {nx} values")
    if out is None:
        out = torch.zeros(nx * ny, dtype=torch.float64, device=census.device)
    elif out.dtype != torch.float64 or out.numel() != nx * ny or not out.is_contiguous():
        raise ValueError(f"out holds {out.numel()} {out.dtype} values: the bounds are {ny} * {nx} float64")
    stats = BoundsStats()
    code = _lib.neutral_hip_window_bounds(nx, ny, C.c_void_p(census.data_ptr()), float(target_population),
                                          float(upper_ratio), float(floor_ratio), int(min_count),
                                          C.c_void_p(out.data_ptr()), C.byref(stats))
    if code != 0:
        raise BoundsRefused(code, stats)
    return out, stats


GROUPS_MAX = 64  # kSpectrumMaxGroups


def group_edges(edges) -> np.ndarray:
    """The G + 1 edges of 1 .. 64 energy groups as the grouped census and window take them: a
    float64 array, every edge finite and > 0, strictly ascending.  Raises ValueError otherwise (the
    library is not touched)."""
    try:
        e = np.ascontiguousarray(edges, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"energy group edges {edges!r} are not numbers") from None
    if e.ndim != 1 or not 2 <= e.size <= GROUPS_MAX + 1:
        raise ValueError(f"energy groups need 2 to {GROUPS_MAX + 1} edges in one row, not shape {e.shape}")
    if not (np.all(np.isfinite(e)) and np.all(e > 0.0) and np.all(e[1:] > e[:-1])):
        raise ValueError("energy group edges are finite, > 0 and strictly ascending")
    return e


def _group_bins(nx, ny, e):
    """-> (nx, ny, G) of a mesh of nx by ny cells under the edges e, small enough for the library"""
    nx, ny = _mesh_size(nx, ny)
    ngroups = e.size - 1
    if not nx * ny * ngroups < 2 ** 30:
        raise ValueError(f"no mesh of {nx} x {ny} cells in {ngroups} groups")
    return nx, ny, ngroups


def census_tally_groups(particles, n: int, nx: int, ny: int, edges, out=None):
    """The census tally over (cell, energy group) bins (include/neutral_hip.h:
    neutral_hip_census_tally_groups): -> (count, weight, stats), two float64 device tensors of
    G * ny * nx values -- G meshes back to back -- and GroupCensusStats.  edges: G + 1 ascending
    energies; a live slot in no group scores nowhere and is counted in stats.outside.  out: a
    float64 device tensor of 2 * G * ny * nx values to tally into; None: a new one.  Otherwise as
    census_tally; raises CensusRefused where the library tallies nothing."""
    e = group_edges(edges)
    _checked(("particle count", n, _COUNT, f"no store holds {n} particles"), particles=particles)
    empty_shard = int(n) == 0 and _lib.neutral_hip_comm_nranks() > 1 and _lib.neutral_hip_store_count(particles) == 0
    if int(n) == 0 and not empty_shard:
        raise ValueError(f"no store holds {n} particles")
    nx, ny, ngroups = _group_bins(nx, ny, e)
    bins = ngroups * nx * ny
    if out is None:
        out = torch.empty(2 * bins, dtype=torch.float64, device="cuda")
    elif out.dtype != torch.float64 or out.numel() != 2 * bins or not out.is_contiguous():
        raise ValueError(f"out holds {out.numel()} {out.dtype} values: the census needs "
                         f"2 * {ngroups} * {ny} * {nx} float64")
    stats = GroupCensusStats()
    code = _lib.neutral_hip_census_tally_groups(particles, int(n), nx, ny, ngroups,
                                                e.ctypes.data_as(C.POINTER(C.c_double)),
                                                C.c_void_p(out.data_ptr()), C.byref(stats))
    if code != 0:
        raise CensusRefused(code, stats)
    return out[:bins], out[bins:], stats


def window_particles_groups(particles, n: int, nx: int, ny: int, edges, lower, upper_ratio: float,
                            survival_ratio: float, max_split: int, seed: int) -> GroupWindowStats:
    """The census weight window over (cell, energy group) bins (include/neutral_hip.h:
    neutral_hip_window_particles_groups): window_particles with a bound for every bin.  edges: G + 1
    ascending energies; `lower` is a device pointer to G * ny * nx doubles, G meshes back to back.
    A live slot in no group has no window and is counted in stats.outside.  Raises WindowRefused
    where the library changes nothing."""
    e = group_edges(edges)
    _checked(("particle count", n, _POSITIVE, f"no store holds {n} particles"),
             ("split limit", max_split, _INT32, f"max_split {max_split} is not an int"),
             ("seed", seed, _UINT64, f"seed {seed} is not a uint64"), particles=particles)
    nx, ny, ngroups = _group_bins(nx, ny, e)
    stats = GroupWindowStats()
    code = _lib.neutral_hip_window_particles_groups(
        particles, int(n), nx, ny, ngroups, e.ctypes.data_as(C.POINTER(C.c_double)), lower,
        float(upper_ratio), float(survival_ratio), int(max_split), int(seed), C.byref(stats))
    if code != 0:
        raise WindowRefused(code, stats)
    return stats


def window_block(block):
    """(block_x, block_y) of a coarse window mesh from one int (both) or a pair: integers >= 1.
    Raises TypeError / ValueError otherwise (the library is not touched)."""
    pair = tuple(block) if isinstance(block, (tuple, list, np.ndarray)) else (block, block)
    if len(pair) != 2:
        raise ValueError(f"a block is one int or (block_x, block_y), not {block!r}")
    bx, by = pair
    _checked(("block width", bx, _POSITIVE, f"no blocks of {bx} x {by} cells"),
             ("block height", by, _POSITIVE, f"no blocks of {bx} x {by} cells"))
    return int(bx), int(by)


def block_bins(nx: int, ny: int, block, edges=None):
    """-> (cnx, cny, G) of the coarse mesh that blocks of `block` cells make of a mesh of nx by ny
    (cnx = ceil(nx / block_x), cny = ceil(ny / block_y)) under the edges (None: no groups, G = 0),
    small enough for the library: max(G, 1) * cnx * cny bins."""
    bx, by = window_block(block)
    nx, ny = _mesh_size(nx, ny)
    ngroups = 0 if edges is None else group_edges(edges).size - 1
    cnx, cny = -(-nx // bx), -(-ny // by)
    return cnx, cny, ngroups


def census_tally_blocks(particles, n: int, nx: int, ny: int, block, edges=None, out=None):
    """The census tally over blocks of cells (include/neutral_hip.h: neutral_hip_census_tally_blocks):
    -> (count, weight, stats), two float64 device tensors of B = max(G, 1) * cny * cnx values --
    max(G, 1) coarse meshes back to back -- and BlockCensusStats.  block: (block_x, block_y) or one
    int for both; edges: G + 1 ascending energies, or None for no groups.  The cells are checked on
    the true mesh of nx by ny.  out: a float64 device tensor of 2 * B values to tally into; None: a
    new one.  Otherwise as census_tally; raises CensusRefused where the library tallies nothing."""
    bx, by = window_block(block)
    e = None if edges is None else group_edges(edges)
    _checked(("particle count", n, _COUNT, f"no store holds {n} particles"), particles=particles)
    empty_shard = int(n) == 0 and _lib.neutral_hip_comm_nranks() > 1 and _lib.neutral_hip_store_count(particles) == 0
    if int(n) == 0 and not empty_shard:
        raise ValueError(f"no store holds {n} particles")
    cnx, cny, ngroups = block_bins(nx, ny, (bx, by), e)
    bins = max(ngroups, 1) * cnx * cny
    if out is None:
        out = torch.empty(2 * bins, dtype=torch.float64, device="cuda")
    elif out.dtype != torch.float64 or out.numel() != 2 * bins or not out.is_contiguous():
        raise ValueError(f"out holds {out.numel()} {out.dtype} values: the census needs "
                         f"2 * {max(ngroups, 1)} * {cny} * {cnx} float64")
    stats = BlockCensusStats()
    code = _lib.neutral_hip_census_tally_blocks(
        particles, int(n), int(nx), int(ny), bx, by, ngroups,
        None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(out.data_ptr()),
        C.byref(stats))
    if code != 0:
        raise CensusRefused(code, stats)
    return out[:bins], out[bins:], stats


def window_particles_blocks(particles, n: int, nx: int, ny: int, block, edges, lower, upper_ratio: float,
                            survival_ratio: float, max_split: int, seed: int) -> GroupWindowStats:
    """The census weight window over blocks of cells (include/neutral_hip.h:
    neutral_hip_window_particles_blocks): window_particles (edges None) or window_particles_groups
    with one bound for every block of `block` cells.  `lower` is a device pointer to
    max(G, 1) * cny * cnx doubles.  Raises WindowRefused where the library changes nothing."""
    bx, by = window_block(block)
    e = None if edges is None else group_edges(edges)
    _checked(("particle count", n, _POSITIVE, f"no store holds {n} particles"),
             ("split limit", max_split, _INT32, f"max_split {max_split} is not an int"),
             ("seed", seed, _UINT64, f"seed {seed} is not a uint64"), particles=particles)
    _, _, ngroups = block_bins(nx, ny, (bx, by), e)
    stats = GroupWindowStats()
    code = _lib.neutral_hip_window_particles_blocks(
        particles, int(n), int(nx), int(ny), bx, by, ngroups,
        None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)), lower,
        float(upper_ratio), float(survival_ratio), int(max_split), int(seed), C.byref(stats))
    if code != 0:
        raise WindowRefused(code, stats)
    return stats


class BatchRefused(Refused):
    """The library folded or computed nothing: code 1 -- an empty array or one of more than 2^30
    entries, a batch number below 1, fewer than 2 batches, a scale that is not finite and positive, a
    batch entry that is not finite, a mean that is not finite, an M2 that is negative or not finite.
    What was to be written is untouched."""
    code_1 = otherwise = ("batch refused: 1 to 2^30 finite entries, batch numbers from 1, at least 2 batches, "
                          "a finite positive scale, moments that are finite with M2 not negative")


def _batch_array(name, a, numel=None):
    if not hasattr(a, "data_ptr") or a.dtype != torch.float64 or not a.is_contiguous():
        raise ValueError(f"{name} is a contiguous float64 device tensor")
    if numel is not None and a.numel() != numel:
        raise ValueError(f"{name} holds {a.numel()} values, not {numel}")
    return a


def _batch_count(name, v):
    _checked((name, v, _INT32, f"{name} {v} is not an int"))
    return int(v)


def batch_fold(x, k: int, moments=None):
    """Folds batch number k (from 1) into running moments (include/neutral_hip.h:
    neutral_hip_batch_fold): -> (moments, stats), a float64 device tensor of 2 * len values -- the
    means of the len entries of x, then their M2 -- and BatchFoldStats.  x: any contiguous float64
    device tensor, a tally as one batch left it.  moments: the tensor of the batches before; None (k
    == 1 alone): a new one.  k == 1 ignores what moments held.  Raises BatchRefused, a ValueError,
    where the library folds nothing (moments is then untouched)."""
    k = _batch_count("batch number", k)
    x = _batch_array("x", x)
    if moments is None:
        if k != 1:
            raise ValueError(f"batch {k} has no moments to be folded into")
        moments = torch.empty(2 * x.numel(), dtype=torch.float64, device=x.device)
    _batch_array("moments", moments, 2 * x.numel())
    stats = BatchFoldStats()
    code = _lib.neutral_hip_batch_fold(C.c_void_p(x.data_ptr()), x.numel(), k, C.c_void_p(moments.data_ptr()),
                                       C.byref(stats))
    if code != 0:
        raise BatchRefused(code, stats)
    return moments, stats


def batch_statistics(moments, nbatches: int, scale: Optional[float] = None, estimate=None, relerr=None):
    """The estimate and its relative error from the moments of nbatches batches (include/neutral_hip.h:
    neutral_hip_batch_statistics): -> (estimate, relerr, stats), two float64 device tensors of len
    values -- scale times the batch mean, and the standard error of the batch mean over its size, 0
    where the mean is 0 -- and BatchStats.  scale: None is nbatches, the tally of all the batches
    together.  estimate, relerr: the tensors to write to; None: new ones.  Raises BatchRefused, a
    ValueError, where the library computes nothing (both are then untouched)."""
    nbatches = _batch_count("number of batches", nbatches)
    moments = _batch_array("moments", moments)
    if moments.numel() % 2:
        raise ValueError(f"moments holds {moments.numel()} values: means, then as many M2")
    n = moments.numel() // 2
    if estimate is None:
        estimate = torch.zeros(n, dtype=torch.float64, device=moments.device)
    if relerr is None:
        relerr = torch.zeros(n, dtype=torch.float64, device=moments.device)
    _batch_array("estimate", estimate, n)
    _batch_array("relerr", relerr, n)
    stats = BatchStats()
    code = _lib.neutral_hip_batch_statistics(
        C.c_void_p(moments.data_ptr()), n, nbatches, float(nbatches if scale is None else scale),
        C.c_void_p(estimate.data_ptr()), C.c_void_p(relerr.data_ptr()), C.byref(stats))
    if code != 0:
        raise BatchRefused(code, stats)
    return estimate, relerr, stats


SPECTRUM_MAX_GROUPS = 64
_WHOLE_MESH = (0, 0, 2**31 - 1, 2**31 - 1)  # (a box beyond the mesh covers the cells it contains)


def set_spectrum_tally(edges, box=None, out=None) -> None:
    """Energy-group flux spectrum over a box of cells for the following steps
    (include/neutral_hip.h): out -- a float64 device tensor (or address) of 2 * ngroups values,
    ngroups = len(edges) - 1 -- receives the track-length estimator by group, then the collision
    estimator.  box = (x0, y0, x1, y1) in global cells, half-open; None: the whole mesh.
    out=None turns the spectrum off.  Raises ValueError, and changes nothing, where the library
    refuses: ngroups outside 1..64, an edge not finite or not positive, edges not strictly
    ascending, an empty box or one with a negative origin."""
    if out is None:
        _lib.neutral_hip_set_spectrum_tally(0, None, 0, 0, 0, 0, None)
        return
    e = np.ascontiguousarray(edges, dtype=np.float64).ravel()
    x0, y0, x1, y1 = (int(v) for v in (box if box is not None else _WHOLE_MESH))
    if hasattr(out, "numel") and out.numel() < 2 * (len(e) - 1):
        raise ValueError(f"out holds {out.numel()} values, the spectrum needs 2 * {len(e) - 1}")
    ptr = _device_address(out)
    if len(e) < 2 or _lib.neutral_hip_set_spectrum_tally(
            len(e) - 1, e.ctypes.data_as(C.POINTER(C.c_double)), x0, y0, x1, y1, C.c_void_p(ptr)) != 0:
        raise ValueError(f"spectrum with {len(e) - 1} groups over box {(x0, y0, x1, y1)} refused: "
                         f"1..{SPECTRUM_MAX_GROUPS} groups, finite positive strictly ascending "
                         "edges, a non-empty box with a non-negative origin")


LEAKAGE_MAX_COSINES = 64


def leakage_shape(edges, ncosines):
    """(4, G + 1, M): the sides, the groups of `edges` (None or empty: none) and the row "no group",
    the cosine bins"""
    e = () if edges is None else np.asarray(edges, dtype=np.float64).ravel()
    return (4, max(len(e) - 1, 0) + 1, int(ncosines))


def set_leakage_tally(edges=None, ncosines=1, out=None) -> None:
    """The leakage tally for the following steps (include/neutral_hip.h): the escapes through the
    vacuum sides by side, energy group and exit cosine.  out -- a float64 device tensor (or address)
    of 2 * 4 * (G + 1) * ncosines values, G = len(edges) - 1 (edges None or empty: G = 0) -- receives
    the weights over N, then the counts, each shaped leakage_shape(edges, ncosines).  out=None turns
    it off.  Raises ValueError, and changes nothing, where the library refuses: more than 64 groups,
    a single edge, an edge not finite or not positive, edges not strictly ascending, ncosines
    outside 1..64."""
    if out is None:
        _lib.neutral_hip_set_leakage_tally(0, None, 1, None)
        return
    e = np.ascontiguousarray(() if edges is None else edges, dtype=np.float64).ravel()
    ngroups = len(e) - 1 if len(e) else 0
    m = int(ncosines)
    if hasattr(out, "numel") and 1 <= m <= LEAKAGE_MAX_COSINES and out.numel() < 8 * (ngroups + 1) * m:
        raise ValueError(f"out holds {out.numel()} values, the leakage tally needs 2 * 4 * {ngroups + 1} * {m}")
    ptr = _device_address(out)
    if (len(e) == 1 or not -2**31 <= m < 2**31 or _lib.neutral_hip_set_leakage_tally(
            ngroups, e.ctypes.data_as(C.POINTER(C.c_double)) if len(e) else None, m, C.c_void_p(ptr)) != 0):
        raise ValueError(f"leakage tally with {ngroups} groups and {m} cosine bins refused: 0..{SPECTRUM_MAX_GROUPS} "
                         f"groups, finite positive strictly ascending edges, 1..{LEAKAGE_MAX_COSINES} cosine bins")


ARITH_AUTO, ARITH_CHECKED = 0, 1


def set_arithmetic(mode: int) -> None:
    """ARITH_AUTO: the device picks the fast or the IEEE-checked kernels per step from the
    step's density mesh and tables; ARITH_CHECKED: always the checked ones."""
    if _lib.neutral_hip_set_arithmetic(mode) != 0:
        raise ValueError(f"unknown arithmetic mode {mode}")


def set_quiet(quiet: bool) -> None:
    _lib.neutral_hip_set_quiet(1 if quiet else 0)


def set_tests_file(path: str) -> None:
    _lib.neutral_hip_set_tests_file(path.encode())


def set_lazy_export(lazy: bool) -> None:
    _lib.neutral_hip_set_lazy_export(1 if lazy else 0)


def set_stream_queues(on: bool) -> None:
    """Tiled variant: migrants change tiles inside the stream kernel (include/neutral_hip.h)."""
    if hasattr(_lib, "neutral_hip_set_stream_queues"):
        _lib.neutral_hip_set_stream_queues(1 if on else 0)


def comm_start() -> int:
    """Joins the ranks named by RANK / WORLD_SIZE / LOCAL_RANK / MASTER_* and brings up
    the tally exchange on the current device; returns COMM_NONE / COMM_RCCL / COMM_HOST."""
    return _lib.neutral_hip_comm_start()


def last_step() -> StepStats:
    s = StepStats()
    _lib.neutral_hip_last_step(C.byref(s))
    return s


def to_host(device_ptr: int, n: int, dtype) -> np.ndarray:
    out = np.empty(n, dtype=dtype)
    if n:
        _lib.neutral_hip_memcpy_d2h(out.ctypes.data, C.c_void_p(device_ptr), out.nbytes)
    return out


def probe_threefry(counter_pkey_mkey: np.ndarray):
    """rows {counter, pkey, master_key} -> (words [n,2] uint64, rn [n,2] float64)"""
    a = np.ascontiguousarray(counter_pkey_mkey, dtype=np.uint64).reshape(-1, 3)
    n = a.shape[0]
    words = np.zeros((n, 2), dtype=np.uint64)
    rn = np.zeros((n, 2), dtype=np.float64)
    _lib.neutral_hip_probe_threefry(a.ctypes.data, words.ctypes.data, rn.ctypes.data, n)
    return words, rn


def probe_cs_lookup(cs: CrossSection, energies: np.ndarray, use_index: bool = True):
    e = np.ascontiguousarray(energies, dtype=np.float64)
    value = np.zeros(e.size, dtype=np.float64)
    index = np.zeros(e.size, dtype=np.int32)
    _lib.neutral_hip_probe_cs_lookup(C.byref(cs), e.ctypes.data, value.ctypes.data,
                                     index.ctypes.data, e.size, 1 if use_index else 0)
    return value, index


def probe_division(rows: np.ndarray):
    """rows {a, b} -> (a / b, quotient through the kept reciprocal, in-range flag)"""
    a = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((a.shape[0], 2), dtype=np.float64)
    plain = np.zeros(a.shape[0], dtype=np.int32)
    _lib.neutral_hip_probe_division(a.ctypes.data, out.ctypes.data, plain.ctypes.data,
                                    a.shape[0])
    return out[:, 0], out[:, 1], plain.astype(bool)


def probe_scatter(rows: np.ndarray):
    """rows {energy, mu_cm, omega_x, omega_y} -> dict of the scatter's kinematics the fast kernels' way and
    with IEEE divisions and roots (include/neutral_hip.h: neutral_hip_probe_scatter)"""
    a = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 4)
    out = np.zeros((a.shape[0], 10), dtype=np.float64)
    _lib.neutral_hip_probe_scatter(a.ctypes.data, out.ctypes.data, a.shape[0])
    names = ("e_new", "cos_fast", "cos_ieee", "speed_fast", "speed_ieee", "u_x_inv_fast", "u_y_inv_fast",
             "u_x_inv_ieee", "u_y_inv_ieee", "cos_checked")
    return {k: out[:, j] for j, k in enumerate(names)}


def probe_policy_quotient(a: np.ndarray, b: np.ndarray):
    """a / b every way the kernels divide (include/neutral_hip.h: neutral_hip_probe_policy_quotient)"""
    rows = np.ascontiguousarray(np.stack([np.asarray(a, dtype=np.float64).ravel(),
                                          np.asarray(b, dtype=np.float64).ravel()], axis=1))
    out = np.zeros((rows.shape[0], 8), dtype=np.float64)
    _lib.neutral_hip_probe_policy_quotient(rows.ctypes.data, out.ctypes.data, rows.shape[0])
    names = ("ieee", "physical_fast", "physical_checked", "mfp_fast", "time_fast", "mfp_checked",
             "time_checked", "rcp_seed")
    return {k: out[:, j] for j, k in enumerate(names)}


def probe_policy_root(x: np.ndarray, energy: np.ndarray):
    """sqrt(x) every way the kernels take it, and the speed of `energy` both ways
    (include/neutral_hip.h: neutral_hip_probe_policy_root)"""
    rows = np.ascontiguousarray(np.stack([np.asarray(x, dtype=np.float64).ravel(),
                                          np.asarray(energy, dtype=np.float64).ravel()], axis=1))
    out = np.zeros((rows.shape[0], 10), dtype=np.float64)
    _lib.neutral_hip_probe_policy_root(rows.ctypes.data, out.ctypes.data, rows.shape[0])
    names = ("ieee", "physical_fast", "physical_checked", "sine_fast", "sine_checked", "rsq_seed",
             "speed_fast", "speed_checked", "speed_arg", "speed_rsq_seed")
    return {k: out[:, j] for j, k in enumerate(names)}


def probe_log(x: np.ndarray):
    """x -> (the kernels' log of a sample, the device library's log)"""
    a = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.zeros((2 * a.size, 4), dtype=np.float64)
    _lib.neutral_hip_probe_log(a.ctypes.data, out.ctypes.data, a.size)
    return out[:a.size, 0], out[:a.size, 1]


def probe_sqrt(x: np.ndarray):
    """x -> (the kernels' square root, the compiler's sqrt)"""
    a = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.zeros((2 * a.size, 4), dtype=np.float64)
    _lib.neutral_hip_probe_log(a.ctypes.data, out.ctypes.data, a.size)
    return out[:a.size, 2], out[:a.size, 3]


def probe_constant_quotients(x: np.ndarray):
    """x -> (x / PARTICLE_MASS kernels' way, compiler's, x / (MASS_NO+1)^2 kernels' way, compiler's)"""
    a = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.zeros((2 * a.size, 4), dtype=np.float64)
    _lib.neutral_hip_probe_log(a.ctypes.data, out.ctypes.data, a.size)
    q = out[a.size:]
    return q[:, 0], q[:, 1], q[:, 2], q[:, 3]


def probe_distance_to_facet(rows: np.ndarray):
    """rows {x, y, omega_x, omega_y, speed, ex_lo, ex_hi, ey_lo, ey_hi}"""
    a = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 9)
    dist = np.zeros(a.shape[0], dtype=np.float64)
    xf = np.zeros(a.shape[0], dtype=np.int32)
    _lib.neutral_hip_probe_distance_to_facet(a.ctypes.data, dist.ctypes.data,
                                             xf.ctypes.data, a.shape[0])
    return dist, xf


@dataclass
class StepResult:
    nprocessed: int
    facets: int
    collisions: int
    kernel_ms: float
    census: int = 0
    stats: Optional["StepStats"] = None
    escape: Optional["EscapeStats"] = None  # the step's escapes through vacuum sides (all zero without any)
    step_claimed: int = 0   # the escape bank: indexes this step's escapes claimed on this rank ...
    step_recorded: int = 0  # ... and records it wrote (both 0 without a bank)
    wraps: Optional["WrapStats"] = None  # the step's wraps through periodic axes (all zero without any)

    @property
    def particle_steps(self) -> int:
        """trips of the event loop (omp3/neutral.c:134): facets + collisions + census"""
        return self.facets + self.collisions + self.census


class Simulation:
    """Device-side state of one problem (or one particle shard of it).

    `shard = (first, count)` makes this process own global particles
    [first, first+count); the RNG key of local particle i is first + i, so any
    partition reproduces the single-GPU histories.
    """

    def __init__(self, problem, cs_keys, cs_values, device: int = 0, shard=None,
                 cs_absorb=None, variant: Optional[int] = None, scalar_flux: bool = False,
                 domain=None, collision_tallies: bool = False, roulette=None, spectrum=None,
                 current: bool = False, outflow: bool = False, vacuum=None, leakage=None,
                 escape_bank: Optional[int] = None, periodic=None):
        import torch

        # periodic: the axes whose outer sides are one seam during this Simulation's steps
        # (periodic_mask: "x", "xy", a mask; None: none)
        self.periodic = periodic_mask(periodic)

        # vacuum: the outer sides histories escape through during this Simulation's steps
        # (vacuum_mask: "wn", "all", a mask; None: every wall reflects)
        self.vacuum = vacuum_mask(vacuum)
        if self.vacuum & periodic_sides(self.periodic):
            # (the library would refuse it at the first step: said here, where the two are named)
            raise ValueError(f"vacuum {vacuum!r} names a side of a periodic axis ({periodic!r}): a wall wraps or "
                             "leaks, not both")
        if not torch.cuda.is_available():
            raise RuntimeError("neutral_amd.interface.Simulation needs a GPU")
        self.torch = torch
        self.p = problem
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        set_device(device)
        set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        self.variant = variant
        # roulette = (weight_cutoff, survival_weight): this Simulation's steps play Russian
        # roulette (set_roulette); None: they run with whatever the library is set to
        self.in_step_window = None  # (window_in_step: the mesh in force during this Simulation's steps)
        self.roulette = None
        if roulette is not None:
            wc, ws = (float(v) for v in roulette)
            previous = _roulette
            set_roulette(wc, ws)  # (refused values raise here)
            set_roulette(*previous)
            self.roulette = (wc, ws)
        if variant is not None:
            set_variant(variant)
        # shard = (first, count): this process owns those global ids (the caller shards);
        # None: all of them -- or, when the rank layer is up (comm_start) with several
        # ranks, the share inject_particles cuts for this rank
        first, count = shard if shard is not None else (0, problem.nparticles)
        self.pid_base, self.n = int(first), int(count)
        self.explicit_shard = shard is not None

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)

        # domain = (ranks_x, ranks_y): spatial decomposition over the ranks of the rank
        # layer (comm_start first).  This rank then holds one block of the mesh -- its
        # edges, density and tally -- and whatever particles are inside it.
        self.domain = domain
        self.x_off, self.y_off, self.lnx, self.lny = problem.x_off, problem.y_off, problem.nx, \
            problem.ny
        if domain is not None:
            xo, yo, lx, ly = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            if _lib.neutral_hip_set_decomposition(domain[0], domain[1], problem.nx, problem.ny,
                                                  C.byref(xo), C.byref(yo), C.byref(lx),
                                                  C.byref(ly)) != 0:
                raise ValueError(f"decomposition {domain} does not fit the ranks or the mesh")
            self.x_off, self.y_off, self.lnx, self.lny = xo.value, yo.value, lx.value, ly.value
            _lib.neutral_hip_set_source_box(problem.local_particle_left_off,
                                            problem.local_particle_bottom_off,
                                            problem.local_particle_width,
                                            problem.local_particle_height)
        bx = slice(self.x_off, self.x_off + self.lnx + 1)
        by = slice(self.y_off, self.y_off + self.lny + 1)
        self.edgex, self.edgey = dev(problem.edgex[bx]), dev(problem.edgey[by])
        self.edgedx, self.edgedy = dev(problem.edgedx[bx]), dev(problem.edgedy[by])
        block = np.asarray(problem.density).reshape(problem.ny, problem.nx)[
            self.y_off:self.y_off + self.lny, self.x_off:self.x_off + self.lnx]
        self.density = dev(block.ravel())
        self.tally = torch.zeros(self.lnx * self.lny, dtype=torch.float64, device=self.device)
        # scalar-flux tally (include/neutral_hip.h): optional second mesh
        self.flux = torch.zeros(self.lnx * self.lny, dtype=torch.float64,
                                device=self.device) if scalar_flux else None
        # collision tallies (include/neutral_hip.h): collisions and absorbed weight per cell
        self.collisions, self.absorbed = (
            torch.zeros(self.lnx * self.lny, dtype=torch.float64, device=self.device)
            for _ in range(2)) if collision_tallies else (None, None)
        # net current (include/neutral_hip.h): Jx and Jy per cell
        self.jx, self.jy = (
            torch.zeros(self.lnx * self.lny, dtype=torch.float64, device=self.device)
            for _ in range(2)) if current else (None, None)
        # outflow (include/neutral_hip.h): weight out of each cell by side, four meshes in one buffer
        self.outflow = torch.zeros(4 * self.lnx * self.lny, dtype=torch.float64,
                                   device=self.device) if outflow else None
        # spectrum = (edges, box): the energy-group flux spectrum over box (global cells, half-open;
        # None: the whole mesh) -- track length by group, then collision (include/neutral_hip.h)
        self.spectrum = None
        if spectrum is not None:
            edges, box = spectrum
            edges = np.ascontiguousarray(edges, dtype=np.float64).ravel()
            box = tuple(int(v) for v in box) if box is not None else (0, 0, problem.nx, problem.ny)
            if not (0 <= box[0] < box[2] <= problem.nx and 0 <= box[1] < box[3] <= problem.ny):
                raise ValueError(f"spectrum box {box} lies outside the {problem.nx} x {problem.ny} mesh")
            self.spectrum = torch.zeros(2 * max(len(edges) - 1, 0), dtype=torch.float64, device=self.device)
            self.spectrum_edges, self.spectrum_box = edges, box
            set_spectrum_tally(edges, box, self.spectrum)  # (refused values raise here)
            set_spectrum_tally(None)
        # leakage = (edges or None, ncosines): the escapes through the vacuum sides by side, energy
        # group and exit cosine -- the weights, then the counts (include/neutral_hip.h)
        self.leakage = None
        if leakage is not None:
            edges, ncosines = leakage
            edges = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).ravel()
            self.leakage_edges, self.leakage_cosines = edges, int(ncosines)
            if not 1 <= self.leakage_cosines <= LEAKAGE_MAX_COSINES:
                raise ValueError(f"leakage tally with {ncosines} cosine bins: 1..{LEAKAGE_MAX_COSINES}")
            self.leakage_shape = leakage_shape(edges, self.leakage_cosines)
            self.leakage = torch.zeros(2 * int(np.prod(self.leakage_shape)), dtype=torch.float64, device=self.device)
            try:
                set_leakage_tally(edges, self.leakage_cosines, self.leakage)  # (refused values raise here)
            finally:
                set_leakage_tally(out=None)
        # escape_bank = capacity: the histories that escape through the vacuum sides during this
        # Simulation's steps are kept, 64 bytes each, in a tensor of its own (include/neutral_hip.h:
        # neutral_hip_set_escape_bank).  The bank accumulates over the steps until reset_escape_bank();
        # it starts over when another Simulation has stepped with a bank in between.
        self.escape_bank = None
        self.escape_bank_on = escape_bank is not None  # (False: the following steps record nothing)
        if escape_bank is not None:
            _checked(("capacity", escape_bank, (1, 2 ** 58), f"an escape bank holds at least one record, not {escape_bank}"))
            self.escape_bank_capacity = int(escape_bank)
            self.escape_bank = torch.zeros(64 * self.escape_bank_capacity, dtype=torch.uint8, device=self.device)
        self._sk, self._sv = dev(cs_keys), dev(cs_values)
        self._cs_keys = np.array(cs_keys, dtype=np.float64)  # (host copy: SourceDescription.check)
        if cs_absorb is None:
            # two separate device copies, as neutral_data.c:176-177 reads both files
            self._ak, self._av = dev(cs_keys), dev(cs_values)
        else:
            self._ak, self._av = dev(cs_absorb[0]), dev(cs_absorb[1])
        self.cs_scatter = CrossSection(self._sk.data_ptr(), self._sv.data_ptr(), len(cs_keys))
        self.cs_absorb = CrossSection(self._ak.data_ptr(), self._av.data_ptr(),
                                      self._ak.numel())
        self.particles = None
        self.nlocal = C.c_int(self.n)
        self.bytes_allocated = 0
        self.last_master_key = 0  # (of the last step(): emit's default seed follows it)

    def _inject_args(self):
        p = self.p
        return (self.lnx, self.lny, p.pad, p.local_particle_left_off, p.local_particle_bottom_off,
                p.local_particle_width, p.local_particle_height, self.x_off, self.y_off, p.dt,
                self.edgex.data_ptr(), self.edgey.data_ptr(), p.initial_energy)

    @staticmethod
    def _source_kind(source):
        """what `source` is taken for: a MeshSource, a BankSource, or else a SourceDescription"""
        for kind in (MeshSource, BankSource):
            if isinstance(source, kind):
                return kind
        return SourceDescription

    def _emit_from(self, count, weight, seed, source):
        """the described or the mesh source out of a source object, which says what is called, what
        comes back and what is raised; refused before anything is written where that can be known"""
        kind = self._source_kind(source)
        if not isinstance(source, kind):
            raise TypeError(f"a source is a SourceDescription, not {type(source).__name__}")
        if self.domain is not None:
            raise kind.refused(2, kind.stats())
        source.check(self.p, self._cs_keys)
        p = self.p
        set_pid_base(self.pid_base)
        return source.emit(self.particles, self.n, count, weight, seed, self.device, self.lnx, self.lny,
                           p.pad, self.x_off, self.y_off, p.dt, self.edgex.data_ptr(),
                           self.edgey.data_ptr())

    def inject(self, source=None):
        """inject_particles on first use, a state reset (no allocation) afterwards.  source = a
        SourceDescription: the initial population comes out of it -- the normal injection, every
        slot marked dead, and the described source with count = n, weight 1 and seed 0, whose
        DescribedSourceStats are returned.  source = a MeshSource: the same with the mesh source
        (source_mesh) and its MeshSourceStats.  What check() refuses is refused before anything is
        written; what the library alone refuses (a share that is negative, a mesh with an entry that
        is negative or not finite, a mesh of zeros) is found after the slots were marked dead: the
        store is then put back to the normal injection before the source's *Refused is raised."""
        if source is None:
            self._inject()
            return None
        kind = self._source_kind(source)  # (refused before anything is written)
        if self.domain is not None:
            raise kind.refused(2, kind.stats())
        if not isinstance(source, kind):
            raise TypeError(f"a source is a SourceDescription, not {type(source).__name__}")
        source.check(self.p, self._cs_keys)
        self._inject()
        dead = self.particles.contents.dead
        _lib.neutral_hip_memset(C.c_void_p(dead), 1, 4 * self.n)  # (every word 0x01010101: dead)
        _lib.neutral_hip_invalidate_particles(self.particles)
        try:
            return self._emit_from(self.n, 1.0, 0, source)
        except kind.refused:
            self._inject()  # (no store of dead slots is left behind)
            raise

    def _inject(self):
        set_pid_base(self.pid_base)
        _lib.neutral_hip_set_auto_shard(0 if self.explicit_shard else 1)
        if self.particles is None:
            p = self.p
            self.particles, self.bytes_allocated = inject_particles(
                self.n, p.nx, *self._inject_args())
            local = _lib.neutral_hip_store_count(self.particles)
            if local >= 0:  # the library cut this rank's share (or block)
                self.n = local
                self.pid_base = int(_lib.neutral_hip_get_pid_base())
                self.nlocal = C.c_int(self.n)
        else:
            _lib.neutral_hip_reinject_particles(self.n, *self._inject_args(), self.particles)
            if self.domain is not None:
                self.n = _lib.neutral_hip_store_count(self.particles)
                self.nlocal = C.c_int(self.n)

    def step(self, master_key: int) -> StepResult:
        # variant and pid base are process-global in the library: re-apply this
        # simulation's own before every call (several Simulations may be alive)
        set_pid_base(self.pid_base)
        if self.variant is not None:
            set_variant(self.variant)
        facets, collisions = C.c_uint64(0), C.c_uint64(0)
        _lib.neutral_hip_set_scalar_flux_tally(
            C.c_void_p(self.flux.data_ptr()) if self.flux is not None else None)
        # (the collision tallies are this Simulation's: set for its step alone, so that no later
        # caller of the library steps into tensors that may be gone by then)
        set_collision_tallies(self.collisions, self.absorbed)
        set_current_tally(self.jx, self.jy)  # (this Simulation's, for its step alone, likewise)
        set_outflow_tally(self.outflow)
        previous_roulette = _roulette
        if self.roulette is not None:
            set_roulette(*self.roulette)
        if self.spectrum is not None:  # (this Simulation's, like the collision tallies)
            set_spectrum_tally(self.spectrum_edges, self.spectrum_box, self.spectrum)
        try:
            if self.in_step_window is not None:  # (this Simulation's, for its step alone, likewise)
                w = self.in_step_window
                set_window_roulette(self.p.nx, self.p.ny, w.lower, w.survival_ratio, w.groups, w.block)
            if self.vacuum:  # (this Simulation's, for its step alone, likewise)
                set_vacuum_sides(self.vacuum)
            if self.periodic:  # (likewise)
                set_periodic_axes(self.periodic)
            if self.leakage is not None:
                set_leakage_tally(self.leakage_edges, self.leakage_cosines, self.leakage)
            self._apply_escape_bank()
            self._solve(master_key, facets, collisions)
        finally:
            if self.leakage is not None:
                set_leakage_tally(out=None)
            if self.periodic:
                set_periodic_axes(0)
            if self.vacuum:
                set_vacuum_sides(0)
            if self.in_step_window is not None:
                set_window_roulette(0, 0, None)
            if self.spectrum is not None:
                set_spectrum_tally(None)
            if self.collisions is not None:
                set_collision_tallies(None, None)
            if self.jx is not None:
                set_current_tally(None, None)
            if self.outflow is not None:
                set_outflow_tally(None)
            if self.roulette is not None:
                set_roulette(*previous_roulette)
        s = last_step()
        self.last_master_key = int(master_key)
        if self.domain is not None:
            self.n = self.nlocal.value  # histories crossed between the ranks' blocks
        bank = escape_bank_stats() if self._bank_mine() else EscapeBankStats()
        return StepResult(int(s.nprocessed), facets.value, collisions.value, s.kernel_ms,
                          int(s.census), s, last_escape(), int(bank.step_claimed), int(bank.step_recorded),
                          last_wraps())

    def _bank_mine(self):
        """is the library's bank this Simulation's"""
        return self.escape_bank is not None and _escape_bank == (self.escape_bank.data_ptr(), self.escape_bank_capacity)

    def _apply_escape_bank(self):
        """The library's bank for this Simulation's step: its own, set when it is not set already (the
        cursor goes on from step to step), or none -- another Simulation's bank is never written to."""
        if self.escape_bank is not None and self.escape_bank_on:
            if not self._bank_mine():
                set_escape_bank(self.escape_bank, self.escape_bank_capacity)
        elif _escape_bank is not None:
            set_escape_bank(None)

    def _solve(self, master_key, facets, collisions):
        p = self.p
        solve_transport_2d(
            self.lnx - 2 * p.pad, self.lny - 2 * p.pad, p.nx, p.ny, master_key, p.pad, self.x_off,
            self.y_off, p.dt, p.nparticles, self.nlocal, None, self.particles,
            self.density.data_ptr(), self.edgex.data_ptr(), self.edgey.data_ptr(),
            self.edgedx.data_ptr(), self.edgedy.data_ptr(), self.cs_scatter,
            self.cs_absorb, self.tally.data_ptr(), None, None, None, facets, collisions)

    def comb(self, seed: int) -> CombStats:
        """Population control at the census (comb_particles): every slot of this Simulation's store
        alive again, at one weight.  Call it between two step()s."""
        if self.particles is None:
            raise RuntimeError("nothing injected yet")
        set_pid_base(self.pid_base)
        return comb_particles(self.particles, self.n, seed)

    def emit(self, count: int, seed: Optional[int] = None, weight: float = 1.0,
             energy: Optional[float] = None, box=None, source=None):
        """The fixed source (source_particles): the first `count` dead slots of this Simulation's
        store become new particles of `weight`.  Call it between two step()s.  box = (left, bottom,
        width, height) and energy default to the problem's own source, seed to 2^63 + the master
        key of the last step().  source = a SourceDescription: the described source
        (source_described) instead, which takes neither energy nor box and returns
        DescribedSourceStats.  source = a MeshSource: the mesh source (source_mesh), likewise, which
        returns MeshSourceStats."""
        if self.particles is None:
            raise RuntimeError("nothing injected yet")
        if seed is None:
            seed = SOURCE_SEED_BASE + self.last_master_key
        if source is not None:
            if energy is not None or box is not None:
                raise ValueError(self._source_kind(source).no_box)
            return self._emit_from(count, weight, seed, source)
        args = list(self._inject_args())
        if box is not None:
            args[3:7] = [float(v) for v in box]
        if energy is not None:
            args[12] = float(energy)
        set_pid_base(self.pid_base)
        return source_particles(self.particles, self.n, count, weight, seed, *args)

    def window(self, lower, upper_ratio: float = 5.0, survival_ratio: float = 3.0, max_split: int = 5,
               seed: Optional[int] = None, groups=None, block=None):
        """The census weight window (window_particles) on this Simulation's store.  Call it between
        two step()s.  `lower` is the mesh of lower weight bounds, (ny, nx) or ny * nx values of the
        global mesh, or one number for a uniform window; 0 means no window in that cell.  seed
        defaults to 2^63 + 2^62 + the master key of the last step().  groups: the G + 1 edges of
        energy groups (group_edges); the window is then window_particles_groups, `lower` is (G, ny,
        nx), G * ny * nx values or one number, and the result a GroupWindowStats.  block: (block_x,
        block_y) or one int for both (window_block); the window is then window_particles_blocks on
        the coarse mesh of cnx by cny blocks, `lower` is (cny, cnx) -- with groups (G, cny, cnx) --,
        as many values flat or one number, and the result a GroupWindowStats."""
        e = None if groups is None else group_edges(groups)
        b = None if block is None else window_block(block)
        if self.particles is None:
            raise RuntimeError("nothing injected yet")
        if self.domain is not None:
            raise WindowRefused(2, WindowStats() if e is None and b is None else GroupWindowStats())
        nx, ny = self.p.nx, self.p.ny
        cnx, cny = (nx, ny) if b is None else block_bins(nx, ny, b)[:2]
        shape = (cny, cnx) if e is None else (e.size - 1, cny, cnx)
        size = int(np.prod(shape))
        mesh = np.asarray(lower, dtype=np.float64)
        if mesh.ndim == 0:
            mesh = np.full(size, float(mesh))
        if mesh.size != size or mesh.shape not in (shape, (size,)):
            raise ValueError(f"lower has shape {mesh.shape}: the mesh is {' x '.join(map(str, shape))}")
        d_lower = torch.from_numpy(np.ascontiguousarray(mesh.ravel())).to(self.device)
        if seed is None:
            seed = WINDOW_SEED_BASE + self.last_master_key
        set_pid_base(self.pid_base)
        if b is not None:
            return window_particles_blocks(self.particles, self.n, nx, ny, b, e, d_lower.data_ptr(), upper_ratio,
                                           survival_ratio, max_split, seed)
        if e is not None:
            return window_particles_groups(self.particles, self.n, nx, ny, e, d_lower.data_ptr(), upper_ratio,
                                           survival_ratio, max_split, seed)
        return window_particles(self.particles, self.n, nx, ny, d_lower.data_ptr(), upper_ratio,
                                survival_ratio, max_split, seed)

    def _window_shape(self, e, b):
        cnx, cny = (self.p.nx, self.p.ny) if b is None else block_bins(self.p.nx, self.p.ny, b)[:2]
        return (cny, cnx) if e is None else (e.size - 1, cny, cnx)

    def window_in_step(self, lower, survival_ratio: float = 3.0, groups=None, block=None):
        """The in-step weight window (set_window_roulette) for this Simulation's following steps:
        an absorption that leaves a weight under lower[bin] plays roulette for survival_ratio *
        lower[bin], where the census window would only see the weight after the step.  `lower`
        takes the shapes window() takes -- the mesh, flat, or one number, of the GLOBAL mesh (also
        with `domain` set) -- or is a float64 device tensor of as many values, which is then read
        where it lies: rewrite it between steps and the next step plays by the new bounds.  None
        turns it off.  groups, block: as window()'s.  The Simulation keeps the device tensor alive.
        Raises ValueError, and keeps the previous setting, where the library refuses -- and for a
        Simulation made with roulette=: the two roulettes are exclusive.
        The Simulation owns the library's setting: this call (to have the mesh checked) and every
        step() put the mesh in force and turn it off again, so a mesh that a caller set with
        set_window_roulette() itself is off afterwards; and every step() has the library check the
        mesh as it then stands, one small reduction kernel and a wait."""
        if lower is None:
            self.in_step_window = None
            return
        if self.roulette is not None and self.roulette[0] > 0.0:
            raise ValueError(f"this Simulation plays roulette with the global cutoff {self.roulette}: "
                             "no in-step window beside it")
        e = None if groups is None else group_edges(groups)
        b = None if block is None else window_block(block)
        shape = self._window_shape(e, b)
        size = int(np.prod(shape))
        if isinstance(lower, torch.Tensor) and lower.is_cuda:
            if lower.dtype != torch.float64 or lower.numel() != size or not lower.is_contiguous():
                raise ValueError(f"lower is not a contiguous float64 tensor of {size} values")
            d_lower = lower
        else:
            mesh = np.asarray(lower, dtype=np.float64)
            if mesh.ndim == 0:
                mesh = np.full(size, float(mesh))
            if mesh.size != size or mesh.shape not in (shape, (size,)):
                raise ValueError(f"lower has shape {mesh.shape}: the mesh is {' x '.join(map(str, shape))}")
            d_lower = torch.from_numpy(np.ascontiguousarray(mesh.ravel())).to(self.device)
        # (the library's verdict now, on the mesh as it stands; in force only during step())
        set_window_roulette(self.p.nx, self.p.ny, d_lower, survival_ratio, e, b)
        set_window_roulette(0, 0, None)
        self.in_step_window = InStepWindow(d_lower, float(survival_ratio), e, b)

    def census(self, out=None, groups=None, block=None):
        """The census tally (census_tally) of this Simulation's store: -> (count, weight, stats), the
        live histories per cell and their weight as float64 device tensors of ny * nx values (the
        global mesh), and CensusStats.  out: a tensor of 2 * ny * nx values to tally into.  Call it
        between two step()s; the store is not written to.  groups: the G + 1 edges of energy groups
        (group_edges); the tally is then census_tally_groups -- G * ny * nx values each, a tensor of
        2 * G * ny * nx to tally into, GroupCensusStats.  block: (block_x, block_y) or one int for
        both (window_block); the tally is then census_tally_blocks over the coarse mesh of cnx by cny
        blocks -- max(G, 1) * cny * cnx values each, BlockCensusStats."""
        e = None if groups is None else group_edges(groups)
        b = None if block is None else window_block(block)
        if self.domain is not None:
            raise CensusRefused(2, BlockCensusStats() if b is not None else
                                CensusStats() if e is None else GroupCensusStats())
        if self.particles is None:
            raise RuntimeError("nothing injected yet")
        meshes = 1 if e is None else e.size - 1
        cnx, cny = (self.p.nx, self.p.ny) if b is None else block_bins(self.p.nx, self.p.ny, b)[:2]
        if out is None:
            out = torch.empty(2 * meshes * cnx * cny, dtype=torch.float64, device=self.device)
        set_pid_base(self.pid_base)
        if b is not None:
            return census_tally_blocks(self.particles, self.n, self.p.nx, self.p.ny, b, e, out)
        if e is not None:
            return census_tally_groups(self.particles, self.n, self.p.nx, self.p.ny, e, out)
        return census_tally(self.particles, self.n, self.p.nx, self.p.ny, out)

    def auto_window(self, target_population: Optional[float] = None, upper_ratio: float = 5.0,
                    survival_ratio: float = 3.0, max_split: int = 5, floor_ratio: float = 0.0,
                    min_count: int = 1, seed: Optional[int] = None, groups=None, block=None,
                    in_step: bool = False):
        """A self-tuning weight window: census(), bounds proportional to the cells' weight
        (window_bounds) for target_population histories (None: the census's live count), then the
        window with them, as window() applies a mesh.  -> (CensusStats, BoundsStats, WindowStats);
        self.last_lower keeps the bounds and self.last_census the two meshes (counts, then
        weights) they were made from, device tensors.  Call it between two step()s.
        groups: the G + 1 edges of energy groups (group_edges).  The three calls then work on the
        (cell, group) bins: the grouped census, window_bounds on it as the census of a mesh of nx by
        G * ny, the grouped window; target_population defaults to the live histories inside the
        groups, live - outside; -> (GroupCensusStats, BoundsStats, GroupWindowStats).
        block: (block_x, block_y) or one int for both (window_block).  The three calls then work on
        the bins of the coarse mesh of cnx by cny blocks, with or without groups: the blocks census,
        window_bounds on it as the census of a mesh of cnx by max(G, 1) * cny, the blocks window;
        -> (BlockCensusStats, BoundsStats, GroupWindowStats).  On a sparse problem, where a cell
        holds one history or none, this is the form that has something to window.
        in_step: the bounds just made (self.last_lower) are also put in force for the following
        steps (window_in_step), with the same groups, block and survival_ratio."""
        e = None if groups is None else group_edges(groups)
        b = None if block is None else window_block(block)
        nx, ny = self.p.nx, self.p.ny
        cnx, cny = (nx, ny) if b is None else block_bins(nx, ny, b)[:2]
        rows = cny if e is None else (e.size - 1) * cny  # (G meshes back to back: one of cnx by G * cny)
        both = torch.empty(2 * cnx * rows, dtype=torch.float64, device=self.device)
        _, _, census = self.census(out=both, groups=e, block=b)
        self.last_census = both  # (counts, then weights: what the bounds were made from)
        if target_population is None:
            found = census if b is None else census.census
            target_population = float(found.live if e is None else found.live - found.outside)
        self.last_lower, bounds = window_bounds(cnx, rows, both, target_population, upper_ratio, floor_ratio,
                                                min_count)
        if in_step:
            self.window_in_step(self.last_lower, survival_ratio, e, b)
        if seed is None:
            seed = WINDOW_SEED_BASE + self.last_master_key
        if self.n == 0:  # (an empty shard among several ranks' took part in the census: nothing to window)
            return census, bounds, WindowStats() if e is None and b is None else GroupWindowStats()
        set_pid_base(self.pid_base)
        if b is not None:
            window = window_particles_blocks(self.particles, self.n, nx, ny, b, e, self.last_lower.data_ptr(),
                                             upper_ratio, survival_ratio, max_split, seed)
        elif e is not None:
            window = window_particles_groups(self.particles, self.n, nx, ny, e, self.last_lower.data_ptr(),
                                             upper_ratio, survival_ratio, max_split, seed)
        else:
            window = window_particles(self.particles, self.n, nx, ny, self.last_lower.data_ptr(), upper_ratio,
                                      survival_ratio, max_split, seed)
        return census, bounds, window

    def particle_keys(self) -> np.ndarray:
        """Global ids of the particles of a decomposed store, in array order."""
        ptr = _lib.neutral_hip_store_keys(self.particles)
        return to_host(ptr, self.n, np.uint32)

    def particle_arrays(self):
        """Host copies of the SoA particle store."""
        _lib.neutral_hip_sync_particles(self.particles)
        pc = self.particles.contents
        out = {}
        for f in F64_FIELDS:
            out[f] = to_host(getattr(pc, f), self.n, np.float64)
        for f in I32_FIELDS:
            out[f] = to_host(getattr(pc, f), self.n, np.int32)
        return out

    def tally_host(self) -> np.ndarray:
        return self.tally.cpu().numpy()

    def collisions_host(self) -> np.ndarray:
        """Collision events per cell (collision_tallies=True)."""
        if self.collisions is None:
            raise RuntimeError("this Simulation keeps no collision tallies")
        return self.collisions.cpu().numpy()

    def absorbed_host(self) -> np.ndarray:
        """Absorbed weight per cell, times 1/N (collision_tallies=True)."""
        if self.absorbed is None:
            raise RuntimeError("this Simulation keeps no collision tallies")
        return self.absorbed.cpu().numpy()

    def current_host(self):
        """(jx, jy): the net current per cell, times 1/N, as (ny, nx) arrays (current=True)."""
        if self.jx is None:
            raise RuntimeError("this Simulation keeps no current")
        return (self.jx.cpu().numpy().reshape(self.lny, self.lnx),
                self.jy.cpu().numpy().reshape(self.lny, self.lnx))

    def outflow_host(self) -> np.ndarray:
        """The outflow per side and cell, times 1/N, as a (4, ny, nx) array: west, east, south,
        north (outflow=True)."""
        if self.outflow is None:
            raise RuntimeError("this Simulation keeps no outflow")
        return self.outflow.cpu().numpy().reshape(4, self.lny, self.lnx)

    def leakage_host(self):
        """(weight, count): the leakage tally's two halves, numpy arrays shaped (4, G + 1, M) -- side,
        group (the last row: no group), cosine bin (leakage=(edges, ncosines))."""
        if self.leakage is None:
            raise RuntimeError("this Simulation keeps no leakage tally")
        v = self.leakage.cpu().numpy()
        n = v.size // 2
        return v[:n].reshape(self.leakage_shape).copy(), v[n:].reshape(self.leakage_shape).copy()

    def _need_bank(self):
        if self.escape_bank is None:
            raise RuntimeError("this Simulation keeps no escape bank")

    def escape_bank_stats(self) -> EscapeBankStats:
        """The bank's capacity, its cursor `claimed`, recorded = min(claimed, capacity), and the last
        step's increments (escape_bank=capacity).  All zero but the capacity before the first step
        and after another Simulation took the library's bank over."""
        self._need_bank()
        return escape_bank_stats() if self._bank_mine() else EscapeBankStats(self.escape_bank_capacity, 0, 0, 0, 0)

    def reset_escape_bank(self) -> None:
        """The cursor back to 0: the next step appends from index 0.  The records stay as they are."""
        self._need_bank()
        if self._bank_mine():
            reset_escape_bank()

    def escape_bank_host(self, lo=None, hi=None) -> np.ndarray:
        """Records lo .. hi - 1 of the bank as a numpy structured array (ESCAPE_RECORD); lo defaults
        to 0, hi to what the bank holds (`recorded`)."""
        self._need_bank()
        lo = 0 if lo is None else int(lo)
        hi = int(self.escape_bank_stats().recorded) if hi is None else int(hi)
        if not 0 <= lo <= hi <= self.escape_bank_capacity:
            raise ValueError(f"records {lo} .. {hi} of a bank of {self.escape_bank_capacity}")
        return self.escape_bank[64 * lo:64 * hi].cpu().numpy().view(ESCAPE_RECORD).copy()

    def sort_escape_bank(self, lo, hi) -> None:
        """Records lo .. hi - 1 put in ascending order of `slot`, on the device (torch: plumbing, no
        kernel of the library's).  The order inside a step's range is whatever the waves' race left;
        sorted by slot -- unique inside a step's range -- a coupled run is reproducible."""
        self._need_bank()
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= self.escape_bank_capacity:
            raise ValueError(f"records {lo} .. {hi} of a bank of {self.escape_bank_capacity}")
        if hi - lo < 2:
            return
        rows = self.escape_bank[64 * lo:64 * hi].view(hi - lo, 64)
        slots = rows[:, 56:60].contiguous().view(self.torch.int32).view(-1).to(self.torch.int64) & 0xFFFFFFFF
        order = self.torch.argsort(slots, stable=True)
        rows.copy_(rows[order])

    def spectrum_host(self):
        """(track, collision): the spectrum's two estimators by group, numpy arrays of ngroups
        (spectrum=(edges, box))."""
        if self.spectrum is None:
            raise RuntimeError("this Simulation keeps no spectrum")
        v = self.spectrum.cpu().numpy()
        g = len(v) // 2
        return v[:g].copy(), v[g:].copy()

    def zero_tally(self):
        self.tally.zero_()
        if self.spectrum is not None:
            self.spectrum.zero_()
        if self.collisions is not None:
            self.collisions.zero_()
            self.absorbed.zero_()
        if self.jx is not None:
            self.jx.zero_()
            self.jy.zero_()
        if self.outflow is not None:
            self.outflow.zero_()
        if self.leakage is not None:
            self.leakage.zero_()

    def validate(self, params_filename: Optional[str] = None):
        validate(self.lnx, self.lny, params_filename or self.p.deck, _lib.neutral_hip_comm_rank(),
                 self.tally.data_ptr())

    def close(self):
        if self.particles is not None:
            _lib.neutral_hip_free_particles(self.particles)
            self.particles = None
        self.jx = self.jy = None  # (the current's meshes go with the Simulation)
        self.outflow = None
        self.in_step_window = None
        if self._bank_mine():
            # (the library is not left pointing at a tensor that goes with this Simulation; a step of
            # any Simulation without a bank turns a bank left behind off as well)
            set_escape_bank(None)
        self.escape_bank = None


@dataclass
class InStepWindow:
    """What Simulation.window_in_step keeps: the mesh on the device and how it is read."""
    lower: "torch.Tensor"
    survival_ratio: float
    groups: Optional[np.ndarray]
    block: Optional[tuple]


@dataclass
class TallyStatistics:
    """One tally of a BatchedRun: what batch_statistics made of its batches."""
    estimate: "torch.Tensor"   # the tally of all the batches together, a device tensor
    relerr: "torch.Tensor"     # per entry: the standard error of the batch mean over its size
    stats: BatchStats
    batch_totals: list         # per batch: nbatches * the sum of its tally (each an estimate of the total)
    total: float               # their mean
    total_se: float            # and its standard error

    @property
    def total_relerr(self) -> float:
        return self.total_se / abs(self.total) if self.total != 0.0 else 0.0


@dataclass
class BatchedResult:
    """What BatchedRun.run returns."""
    nbatches: int
    tallies: dict              # name -> TallyStatistics
    wall_seconds: float
    between: list              # per batch: what the `between` hook returned after each step

    def __getitem__(self, name) -> TallyStatistics:
        return self.tallies[name]

    @property
    def fom(self) -> float:
        """The figure of merit of the energy tally: 1 / (mean relerr^2 * wall seconds)."""
        r = self.tallies["energy"].stats.mean_relerr
        return 1.0 / (r * r * self.wall_seconds) if r > 0.0 and self.wall_seconds > 0.0 else float("inf")


def welford_total(values):
    """(mean, standard error of the mean) of a few host numbers, by the update of
    neutral_hip_batch_fold and the formulas of neutral_hip_batch_statistics."""
    mean, m2 = 0.0, 0.0
    for k, v in enumerate(values, 1):
        d = v - mean
        mean = mean + d / k
        m2 = m2 + d * (v - mean)
    n = len(values)
    return mean, float(np.sqrt(m2 / (n - 1) / n)) if n > 1 else 0.0


class BatchedRun:
    """A run of `batches` independent batches, for a standard error on every tally.

    The N particles are cut into B shards of N / B; one Simulation with shard = (0, N / B) runs
    them one after the other, each through all its steps, its store re-injected with the batch's
    own particle ids.  Every tally is normalised by N, so a batch's tally is its share of the whole
    run's, the B of them are independent, and their sum is the tally of the run (batch_fold,
    batch_statistics).  simulation_options are Simulation's (variant, roulette, the optional
    tallies); shard and domain are not among them."""

    def __init__(self, problem, cs_keys, cs_values, batches: int, **simulation_options):
        batches = _batch_count("number of batches", batches)
        if batches < 2:
            raise ValueError(f"{batches} batch(es) have no spread: at least 2")
        if simulation_options.get("domain") is not None:
            raise ValueError("a decomposed mesh is not run in batches")
        if simulation_options.get("shard") is not None:
            raise ValueError("the batches are the shards: shard= is not an option")
        if problem.nparticles % batches != 0 or problem.nparticles < batches:
            raise ValueError(f"{batches} batches do not divide {problem.nparticles} particles")
        simulation_options.pop("domain", None)
        simulation_options.pop("shard", None)
        self.nbatches = batches
        self.per_batch = problem.nparticles // batches
        self.sim = Simulation(problem, cs_keys, cs_values, shard=(0, self.per_batch), **simulation_options)

    def tallies(self) -> dict:
        """name -> device tensor, of every tally the Simulation keeps"""
        sim = self.sim
        kept = {"energy": sim.tally, "flux": sim.flux, "collisions": sim.collisions, "absorbed": sim.absorbed,
                "jx": sim.jx, "jy": sim.jy, "outflow": sim.outflow, "spectrum": sim.spectrum}
        return {name: t for name, t in kept.items() if t is not None}

    def run(self, steps: int, between=None, each_batch=None) -> BatchedResult:
        """Runs every batch through master keys 1 .. steps.  between(sim, tt) is called after each
        step: the place of sim.auto_window(), sim.comb() or sim.emit(); each_batch(sim, b) after a
        batch's last step, while the tallies hold that batch alone."""
        import time
        sim, nb = self.sim, self.nbatches
        kept = self.tallies()
        moments = {name: torch.empty(2 * t.numel(), dtype=torch.float64, device=sim.device)
                   for name, t in kept.items()}
        sums = {name: [] for name in kept}
        returned = []
        torch.cuda.synchronize(sim.device)
        t0 = time.perf_counter()
        for b in range(nb):
            sim.pid_base = b * self.per_batch
            sim.inject()
            for t in kept.values():
                t.zero_()
            returned.append([])
            for tt in range(1, steps + 1):
                sim.step(tt)
                if between is not None:
                    returned[-1].append(between(sim, tt))
            if each_batch is not None:
                each_batch(sim, b)
            for name, t in kept.items():
                _, fold = batch_fold(t, b + 1, moments[name])
                sums[name].append(fold.sum * nb)
        out = {}
        for name, t in kept.items():
            estimate, relerr, stats = batch_statistics(moments[name], nb)
            total, total_se = welford_total(sums[name])
            out[name] = TallyStatistics(estimate, relerr, stats, sums[name], total, total_se)
        torch.cuda.synchronize(sim.device)
        return BatchedResult(nb, out, time.perf_counter() - t0, returned)

    def close(self):
        self.sim.close()
