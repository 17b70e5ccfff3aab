"""ctypes binding of the C-ABI in include/xfemm_kernels.h (lib/libxfemm_kernels.so).

This is the Python view of the MI355X hot path used by tests and bench.py.
There is no CPU fallback: if the HIP library is missing, or no gfx950 device
is present, every solve raises.
"""
from __future__ import annotations

import ctypes as C
import cmath
import math
import os
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(HERE, "lib")
KERNELS_SO = os.path.join(LIB_DIR, "libxfemm_kernels.so")

dptr = C.POINTER(C.c_double)
iptr = C.POINTER(C.c_int)

XFK_OK = 0
XFK_REBUILD_SYMBOLIC = 1
XFK_TIME_SPMV = 2
XFK_TIME_TAIL = 4
XFK_PRECOND_JACOBI = 0
XFK_PRECOND_AMG = 1
PRECONDS = {"jacobi": XFK_PRECOND_JACOBI, "amg": XFK_PRECOND_AMG}
XFK_OPT_PRECOND = 1
XFK_OPT_AMG_SWEEPS = 2
XFK_OPT_AMG_THETA = 3
XFK_OPT_AMG_OMEGA = 4
XFK_OPT_AMG_REPLICATE = 5
XFK_OPT_AMG_REUSE = 6
XFK_OPT_AMG_DENSE = 7
XFK_OPT_AMG_FOLD = 8
XFK_OPT_AMG_COL16 = 9
XFK_OPT_AMG_WLEVEL = 10
XFK_OPT_AMG_F32 = 11
XFK_OPT_NEWTON_INEXACT = 12
XFK_OPT_HEAT_MAX_PASSES = 13

# every symbol include/xfemm_kernels.h declares
EXPORTED = (
    "xfk_last_error", "xfk_age_element_matrix", "xfk_device_count", "xfk_device_init", "xfk_problem_create", "xfk_problem_destroy",
    "xfk_static2d", "xfk_get_solution", "xfk_get_circuits", "xfk_get_csr", "xfk_get_nnz", "xfk_spmv_col_bytes",
    "xfk_static2d_assemble_at", "xfk_get_element_state",
    "xfk_get_stream", "xfk_pcg_solve_csr", "xfk_pcg_solve_csr_pc", "xfk_pcg_time", "xfk_phase_profile",
    "xfk_alloc_stats", "xfk_problem_memory", "xfk_cache_stats", "xfk_release_cache",
    "xfk_amg_forget_hints",
    "xfk_set_option",
    "xfk_problem_create_harmonic", "xfk_problem_create_harmonic_dist", "xfk_harmonic2d",
    "xfk_get_solution_complex", "xfk_get_circuits_complex",
    "xfk_get_csr_complex",
    "xfk_comm_unique_id", "xfk_comm_create_rccl", "xfk_comm_create_local", "xfk_comm_destroy",
    "xfk_comm_rank", "xfk_comm_size", "xfk_comm_record", "xfk_comm_log", "xfk_comm_create_replay",
    "xfk_comm_time", "xfk_comm_timing",
    "xfk_partition_plan", "xfk_partition_plan_coupled", "xfk_problem_create_dist", "xfk_dist_get_info",
    "xfk_magdir_eval", "xfk_magdir_eval_labels", "xfk_lua_run", "xfk_sort_elements",
    "xfk_problem_create_electrostatic", "xfk_electrostatic", "xfk_get_conductors", "xfk_conductor_charge",
    "xfk_problem_create_heatflow", "xfk_heatflow", "xfk_heatflow_assemble", "xfk_heatflow_set_step",
    "xfk_heatflow_advance", "xfk_hf_get_conductors", "xfk_hf_conductor_flow",
    "xfk_pot_set_solution", "xfk_pot_get_qmarks", "xfk_pot_set_qmarks", "xfk_pot_plot_bounds", "xfk_pot_block_integrals_ordered",
    "xfk_pot_point_values_at", "xfk_pot_element_fields", "xfk_pot_corner_fields", "xfk_pot_corner_branches",
    "xfk_pot_block_integrals", "xfk_pot_block_integral", "xfk_pot_point_values", "xfk_pot_grid_info", "xfk_pot_time",
    "xfk_pot_make_mask", "xfk_pot_get_mask", "xfk_pot_mask_info", "xfk_pot_mask_problem", "xfk_pot_stress_time",
    "xfk_pot_line_integrals", "xfk_pot_line_integral", "xfk_pot_contour_samples", "xfk_pot_contour_time",
    "xfk_mag_set_solution", "xfk_mag_set_depth", "xfk_mag_element_b", "xfk_mag_block_integrals",
    "xfk_mag_block_integral", "xfk_mag_time",
    "xfk_mag_ac_set_solution", "xfk_mag_ac_element_b", "xfk_mag_ac_block_integrals", "xfk_mag_ac_block_integral",
    "xfk_mag_ac_time",
    "xfk_mag_make_mask", "xfk_mag_get_mask", "xfk_mag_mask_info", "xfk_mag_mask_problem", "xfk_mag_stress_time",
    "xfk_mag_corner_b", "xfk_mag_point_values", "xfk_mag_point_values_at", "xfk_mag_line_integrals",
    "xfk_mag_line_integral", "xfk_mag_contour_samples", "xfk_mag_point_time", "xfk_mag_contour_time",
    "xfk_amg_probe_create", "xfk_amg_probe_info", "xfk_amg_probe_level_size", "xfk_amg_probe_level_csr",
    "xfk_amg_probe_tiles", "xfk_amg_probe_vector", "xfk_amg_probe_trace", "xfk_amg_probe_apply",
    "xfk_amg_probe_refresh", "xfk_amg_probe_destroy",
)


class BlockDesc(C.Structure):
    _fields_ = [("mu_x", C.c_double), ("mu_y", C.c_double), ("H_c", C.c_double),
                ("J_re", C.c_double), ("Cduct", C.c_double), ("LamFill", C.c_double),
                ("LamType", C.c_int), ("BHpoints", C.c_int),
                ("B", dptr), ("H", dptr), ("slope", dptr)]


class LabelDesc(C.Structure):
    _fields_ = [("block", C.c_int), ("in_circuit", C.c_int), ("mag_dir", C.c_double),
                ("is_wound", C.c_int), ("is_external", C.c_int), ("mag_dir_fctn", C.c_char_p)]


class LineDesc(C.Structure):
    _fields_ = [("format", C.c_int), ("A0", C.c_double), ("A1", C.c_double), ("A2", C.c_double),
                ("phi", C.c_double), ("c0", C.c_double), ("c1", C.c_double)]


class PointDesc(C.Structure):
    _fields_ = [("A_re", C.c_double), ("A_im", C.c_double), ("J_re", C.c_double),
                ("J_im", C.c_double)]


class CircuitDesc(C.Structure):
    _fields_ = [("type", C.c_int), ("amps_re", C.c_double), ("dvolts_re", C.c_double)]


class AgeDesc(C.Structure):
    """xfk_age_desc: one CAirGapElement as read from the .pbc file."""
    _fields_ = [("format", C.c_int), ("ri", C.c_double), ("ro", C.c_double), ("total_arc_length", C.c_double),
                ("inner_shift", C.c_double), ("outer_shift", C.c_double), ("n_arc", C.c_int),
                ("qn", iptr), ("qw", dptr)]


class ProblemDesc(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("x", dptr), ("y", dptr), ("marker", iptr),
                ("n_elems", C.c_int), ("p", iptr), ("e", iptr), ("lbl", iptr),
                ("n_blocks", C.c_int), ("blocks", C.POINTER(BlockDesc)),
                ("n_labels", C.c_int), ("labels", C.POINTER(LabelDesc)),
                ("n_lines", C.c_int), ("lines", C.POINTER(LineDesc)),
                ("n_points", C.c_int), ("points", C.POINTER(PointDesc)),
                ("n_circs", C.c_int), ("circs", C.POINTER(CircuitDesc)),
                ("n_pbc", C.c_int), ("pbc", iptr),
                ("precision", C.c_double), ("length_units", C.c_int), ("coords", C.c_int),
                ("relax", C.c_double), ("problem_type", C.c_int), ("ext_zo", C.c_double),
                ("ext_ro", C.c_double), ("ext_ri", C.c_double),
                ("n_ages", C.c_int), ("ages", C.POINTER(AgeDesc))]


XFK_PLANAR = 0
XFK_AXISYMMETRIC = 1


class EsBlockDesc(C.Structure):
    _fields_ = [("ex", C.c_double), ("ey", C.c_double), ("qv", C.c_double)]


class EsLabelDesc(C.Structure):
    _fields_ = [("block", C.c_int), ("is_external", C.c_int)]


class EsLineDesc(C.Structure):
    _fields_ = [("format", C.c_int), ("V", C.c_double), ("qs", C.c_double), ("c0", C.c_double), ("c1", C.c_double)]


class EsPointDesc(C.Structure):
    _fields_ = [("V", C.c_double), ("qp", C.c_double)]


class EsConductorDesc(C.Structure):
    _fields_ = [("type", C.c_int), ("V", C.c_double), ("q", C.c_double)]


class EsProblemDesc(C.Structure):
    """xfk_es_problem_desc: the state ESolver::LoadProblemFile / LoadMesh leave behind."""
    _fields_ = [("n_nodes", C.c_int), ("x", dptr), ("y", dptr), ("marker", iptr), ("conductor", iptr),
                ("n_elems", C.c_int), ("p", iptr), ("e", iptr), ("lbl", iptr),
                ("n_blocks", C.c_int), ("blocks", C.POINTER(EsBlockDesc)),
                ("n_labels", C.c_int), ("labels", C.POINTER(EsLabelDesc)),
                ("n_lines", C.c_int), ("lines", C.POINTER(EsLineDesc)),
                ("n_points", C.c_int), ("points", C.POINTER(EsPointDesc)),
                ("n_conductors", C.c_int), ("conductors", C.POINTER(EsConductorDesc)),
                ("n_pbc", C.c_int), ("pbc", iptr),
                ("precision", C.c_double), ("length_units", C.c_int), ("problem_type", C.c_int),
                ("depth", C.c_double), ("ext_zo", C.c_double), ("ext_ro", C.c_double), ("ext_ri", C.c_double)]


class HfBlockDesc(C.Structure):
    _fields_ = [("kx", C.c_double), ("ky", C.c_double), ("kt", C.c_double), ("qv", C.c_double),
                ("npts", C.c_int), ("T", dptr), ("K", dptr)]


class HfLabelDesc(C.Structure):
    _fields_ = [("block", C.c_int), ("is_external", C.c_int)]


class HfLineDesc(C.Structure):
    _fields_ = [("format", C.c_int), ("Tset", C.c_double), ("qs", C.c_double), ("beta", C.c_double),
                ("h", C.c_double), ("Tinf", C.c_double)]


class HfPointDesc(C.Structure):
    _fields_ = [("T", C.c_double), ("qp", C.c_double)]


class HfConductorDesc(C.Structure):
    _fields_ = [("type", C.c_int), ("T", C.c_double), ("q", C.c_double)]


class HfProblemDesc(C.Structure):
    """xfk_hf_problem_desc: the state HSolver::LoadProblemFile / LoadMesh leave behind."""
    _fields_ = [("n_nodes", C.c_int), ("x", dptr), ("y", dptr), ("marker", iptr), ("conductor", iptr),
                ("n_elems", C.c_int), ("p", iptr), ("e", iptr), ("lbl", iptr),
                ("n_blocks", C.c_int), ("blocks", C.POINTER(HfBlockDesc)),
                ("n_labels", C.c_int), ("labels", C.POINTER(HfLabelDesc)),
                ("n_lines", C.c_int), ("lines", C.POINTER(HfLineDesc)),
                ("n_points", C.c_int), ("points", C.POINTER(HfPointDesc)),
                ("n_conductors", C.c_int), ("conductors", C.POINTER(HfConductorDesc)),
                ("n_pbc", C.c_int), ("pbc", iptr),
                ("precision", C.c_double), ("length_units", C.c_int), ("problem_type", C.c_int),
                ("depth", C.c_double), ("ext_zo", C.c_double), ("ext_ro", C.c_double), ("ext_ri", C.c_double),
                ("dt", C.c_double), ("t_prev", dptr)]


class Result(C.Structure):
    _fields_ = [("newton_iters", C.c_int), ("cg_iters", C.c_longlong), ("last_res", C.c_double),
                ("final_er", C.c_double), ("nnz", C.c_longlong), ("ncolors", C.c_int),
                ("ms_symbolic", C.c_double), ("ms_assemble", C.c_double), ("ms_solve", C.c_double),
                ("spmv_ms_avg", C.c_double), ("spmv_samples", C.c_int),
                ("color_rounds", C.c_int), ("precond", C.c_int), ("amg_levels", C.c_int),
                ("amg_op_complexity", C.c_double), ("ms_amg_setup", C.c_double), ("ms_rep_cycle", C.c_double),
                ("rep_cycles", C.c_int), ("ms_rep_setup", C.c_double), ("prec_fallback", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DistInfo(C.Structure):
    _fields_ = [("rank", C.c_int), ("nranks", C.c_int), ("n_global", C.c_int), ("row0", C.c_int),
                ("n_own", C.c_int), ("n_halo", C.c_int), ("n_elems", C.c_int), ("n_send", C.c_int),
                ("n_recv", C.c_int), ("n_extra", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AmgProbeOpts(C.Structure):
    _fields_ = [("sweeps", C.c_int), ("theta", C.c_double), ("omega", C.c_double), ("dense_max", C.c_int),
                ("fold", C.c_int), ("col16", C.c_int), ("f32", C.c_int), ("wlevel", C.c_int)]


class AmgLevelInfo(C.Structure):
    _fields_ = [("n", C.c_int), ("nc", C.c_int), ("fold", C.c_int), ("has16", C.c_int), ("has32", C.c_int),
                ("w_at", C.c_int), ("nnz", C.c_longlong), ("pnnz", C.c_longlong), ("fnnz", C.c_longlong),
                ("weight", C.c_double), ("rho_f", C.c_double)]


class AmgInfo(C.Structure):
    _fields_ = [("levels", C.c_int), ("dense_coarse", C.c_int), ("cinv_f64", C.c_int), ("traced", C.c_int),
                ("level", AmgLevelInfo * 16)]


_lib = None


class XfkError(RuntimeError):
    pass


def load_library(path: str = KERNELS_SO):
    """Load lib/libxfemm_kernels.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise XfkError("HIP library %s not built (run __graft_entry__.build() / make -C xfemm_amd)" % path)
    L = C.CDLL(path)
    L.xfk_last_error.restype = C.c_char_p
    L.xfk_device_count.restype = C.c_int
    L.xfk_problem_create.argtypes = [C.POINTER(ProblemDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.xfk_problem_destroy.argtypes = [C.c_void_p]
    L.xfk_static2d.argtypes = [C.c_void_p, C.c_int, C.POINTER(Result)]
    L.xfk_get_solution.argtypes = [C.c_void_p, dptr]
    L.xfk_get_circuits.argtypes = [C.c_void_p, iptr, dptr, dptr]
    L.xfk_get_csr.argtypes = [C.c_void_p, iptr, iptr, dptr, dptr]
    L.xfk_static2d_assemble_at.argtypes = [C.c_void_p, C.c_int, dptr]
    L.xfk_get_element_state.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_get_nnz.argtypes = [C.c_void_p]
    L.xfk_get_nnz.restype = C.c_longlong
    L.xfk_spmv_col_bytes.argtypes = [C.c_void_p]
    L.xfk_spmv_col_bytes.restype = C.c_double
    L.xfk_get_stream.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.xfk_pcg_solve_csr.argtypes = [C.c_int, iptr, iptr, dptr, dptr, dptr, C.c_int, C.c_double, C.c_int,
                                    C.POINTER(C.c_longlong), dptr]
    L.xfk_pcg_solve_csr_pc.argtypes = [C.c_int, iptr, iptr, dptr, dptr, dptr, C.c_int, C.c_double, C.c_int,
                                       C.c_int, C.POINTER(C.c_longlong), dptr]
    L.xfk_pcg_time.argtypes = [C.c_void_p, C.c_int, dptr, dptr]
    L.xfk_amg_probe_create.argtypes = [C.c_int, iptr, iptr, dptr, C.c_int, C.POINTER(AmgProbeOpts), C.c_int,
                                       C.POINTER(C.c_void_p)]
    L.xfk_amg_probe_info.argtypes = [C.c_void_p, C.POINTER(AmgInfo)]
    L.xfk_amg_probe_level_size.argtypes = [C.c_void_p, C.c_int, C.c_int, iptr, iptr, C.POINTER(C.c_longlong)]
    L.xfk_amg_probe_level_csr.argtypes = [C.c_void_p, C.c_int, C.c_int, iptr, iptr, dptr]
    L.xfk_amg_probe_tiles.argtypes = [C.c_void_p, C.c_int, iptr, iptr]
    L.xfk_amg_probe_vector.argtypes = [C.c_void_p, C.c_int, C.c_int, dptr]
    L.xfk_amg_probe_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.xfk_amg_probe_apply.argtypes = [C.c_void_p, C.c_int, dptr, dptr]
    L.xfk_amg_probe_refresh.argtypes = [C.c_void_p, dptr, C.c_int]
    L.xfk_amg_probe_destroy.argtypes = [C.c_void_p]
    L.xfk_amg_probe_destroy.restype = None
    L.xfk_phase_profile.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.xfk_alloc_stats.argtypes = [dptr, C.c_int]
    L.xfk_problem_memory.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
    L.xfk_cache_stats.argtypes = [C.POINTER(C.c_longlong)]
    L.xfk_set_option.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.xfk_problem_create_harmonic.argtypes = [C.POINTER(ProblemDesc), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    L.xfk_problem_create_harmonic_dist.argtypes = [C.POINTER(ProblemDesc), C.c_void_p, C.c_int, C.c_void_p,
                                                   C.POINTER(C.c_void_p)]
    L.xfk_harmonic2d.argtypes = [C.c_void_p, C.c_int, C.POINTER(Result)]
    L.xfk_get_solution_complex.argtypes = [C.c_void_p, dptr]
    L.xfk_get_circuits_complex.argtypes = [C.c_void_p, iptr, dptr, dptr]
    L.xfk_get_csr_complex.argtypes = [C.c_void_p, iptr, iptr, dptr, dptr]
    L.xfk_age_element_matrix.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, dptr]
    vp = C.c_void_p
    L.xfk_comm_unique_id.argtypes = [C.c_char_p, C.c_int]
    L.xfk_comm_create_rccl.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.xfk_comm_create_local.argtypes = [C.c_int, C.POINTER(vp)]
    L.xfk_comm_destroy.argtypes = [vp]
    L.xfk_comm_rank.argtypes = [vp]
    L.xfk_comm_size.argtypes = [vp]
    L.xfk_comm_record.argtypes = [vp, C.c_int]
    L.xfk_comm_log.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.xfk_comm_time.argtypes = [vp, C.c_int]
    L.xfk_comm_timing.argtypes = [vp, C.POINTER(C.c_longlong), dptr, dptr]
    L.xfk_comm_create_replay.argtypes = [vp, C.POINTER(vp)]
    L.xfk_partition_plan.argtypes = [C.c_int, C.c_int, iptr, C.c_int, C.c_int, C.POINTER(DistInfo),
                                     iptr, iptr, iptr, iptr]
    L.xfk_partition_plan_coupled.argtypes = [C.c_int, C.c_int, iptr, C.c_int, C.c_int, C.c_int, iptr,
                                             C.POINTER(DistInfo), iptr, iptr, iptr, iptr]
    L.xfk_problem_create_dist.argtypes = [C.POINTER(ProblemDesc), C.c_int, vp, C.POINTER(vp)]
    L.xfk_dist_get_info.argtypes = [vp, C.POINTER(DistInfo)]
    L.xfk_problem_create_electrostatic.argtypes = [C.POINTER(EsProblemDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.xfk_electrostatic.argtypes = [C.c_void_p, C.c_int, C.POINTER(Result)]
    L.xfk_get_conductors.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_conductor_charge.argtypes = [C.c_void_p, C.c_int, dptr]
    L.xfk_problem_create_heatflow.argtypes = [C.POINTER(HfProblemDesc), C.c_int, C.POINTER(C.c_void_p)]
    L.xfk_heatflow.argtypes = [C.c_void_p, C.c_int, C.POINTER(Result)]
    L.xfk_heatflow_assemble.argtypes = [C.c_void_p, dptr]
    L.xfk_heatflow_set_step.argtypes = [C.c_void_p, C.c_double, dptr]
    L.xfk_heatflow_advance.argtypes = [C.c_void_p, C.c_double]
    L.xfk_hf_get_conductors.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_hf_conductor_flow.argtypes = [C.c_void_p, C.c_int, dptr]
    ubptr = C.POINTER(C.c_ubyte)
    L.xfk_pot_set_solution.argtypes = [C.c_void_p, dptr]
    L.xfk_pot_get_qmarks.argtypes = [C.c_void_p, iptr]
    L.xfk_pot_set_qmarks.argtypes = [C.c_void_p, iptr]
    L.xfk_pot_plot_bounds.argtypes = [C.c_void_p, dptr]
    L.xfk_pot_block_integrals_ordered.argtypes = [C.c_void_p, ubptr, dptr]
    L.xfk_pot_point_values_at.argtypes = [C.c_void_p, C.c_int, dptr, dptr, iptr, C.c_int, dptr]
    L.xfk_pot_element_fields.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_pot_corner_fields.argtypes = [C.c_void_p, dptr]
    L.xfk_pot_corner_branches.argtypes = [C.c_void_p, ubptr]
    L.xfk_pot_block_integrals.argtypes = [C.c_void_p, ubptr, dptr]
    L.xfk_pot_block_integral.argtypes = [C.c_void_p, ubptr, C.c_int, dptr]
    L.xfk_pot_make_mask.argtypes = [C.c_void_p, ubptr, ubptr, dptr]
    L.xfk_pot_get_mask.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_pot_mask_info.argtypes = [C.c_void_p, dptr]
    L.xfk_pot_mask_problem.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.xfk_pot_stress_time.argtypes = [C.c_void_p, C.c_int, dptr]
    L.xfk_pot_grid_info.argtypes = [C.c_void_p, dptr]
    L.xfk_pot_time.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, dptr, dptr]
    L.xfk_pot_point_values.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, iptr, dptr]
    L.xfk_pot_line_integrals.argtypes = [C.c_void_p, C.c_int, iptr, dptr, dptr, C.c_int, C.c_int, C.c_int, dptr, iptr]
    L.xfk_pot_line_integral.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, C.c_int, C.c_int, dptr, iptr]
    L.xfk_pot_contour_samples.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, C.c_int, dptr, iptr]
    L.xfk_pot_contour_time.argtypes = [C.c_void_p, C.c_int, iptr, dptr, dptr, C.c_int, C.c_int, C.c_int, C.c_int, dptr]
    L.xfk_mag_set_solution.argtypes = [C.c_void_p, dptr]
    L.xfk_mag_set_depth.argtypes = [C.c_void_p, C.c_double]
    L.xfk_mag_element_b.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_mag_block_integrals.argtypes = [C.c_void_p, ubptr, dptr]
    L.xfk_mag_block_integral.argtypes = [C.c_void_p, ubptr, C.c_int, dptr]
    L.xfk_mag_time.argtypes = [C.c_void_p, C.c_int, dptr]
    L.xfk_mag_ac_set_solution.argtypes = [C.c_void_p, dptr]
    L.xfk_mag_ac_element_b.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_mag_ac_block_integrals.argtypes = [C.c_void_p, ubptr, dptr]
    L.xfk_mag_ac_block_integral.argtypes = [C.c_void_p, ubptr, C.c_int, dptr]
    L.xfk_mag_ac_time.argtypes = [C.c_void_p, C.c_int, dptr]
    L.xfk_mag_make_mask.argtypes = [C.c_void_p, ubptr, dptr, ubptr]
    L.xfk_mag_get_mask.argtypes = [C.c_void_p, dptr, dptr]
    L.xfk_mag_mask_info.argtypes = [C.c_void_p, dptr]
    L.xfk_mag_mask_problem.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.xfk_mag_stress_time.argtypes = [C.c_void_p, C.c_int, dptr]
    L.xfk_mag_corner_b.argtypes = [C.c_void_p, dptr]
    L.xfk_mag_point_values.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, iptr, dptr]
    L.xfk_mag_point_values_at.argtypes = [C.c_void_p, C.c_int, dptr, dptr, iptr, C.c_int, dptr]
    L.xfk_mag_line_integrals.argtypes = [C.c_void_p, C.c_int, iptr, dptr, dptr, C.c_int, C.c_int, C.c_int, dptr, iptr]
    L.xfk_mag_line_integral.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, C.c_int, C.c_int, dptr, iptr]
    L.xfk_mag_contour_samples.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, C.c_int, dptr, iptr]
    L.xfk_mag_point_time.argtypes = [C.c_void_p, C.c_int, dptr, dptr, C.c_int, dptr]
    L.xfk_mag_contour_time.argtypes = [C.c_void_p, C.c_int, iptr, dptr, dptr, C.c_int, C.c_int, C.c_int, C.c_int, dptr]
    L.xfk_sort_elements.argtypes = [C.c_int, C.POINTER(C.c_uint), C.c_int, iptr]
    L.xfk_magdir_eval.argtypes = [C.c_char_p, C.c_int, iptr, dptr, dptr, C.c_int, C.c_double, dptr]
    L.xfk_lua_run.argtypes = [C.c_char_p, C.c_char_p, C.c_longlong, C.POINTER(C.c_longlong)]
    L.xfk_magdir_eval_labels.argtypes = [C.c_int, C.POINTER(C.c_char_p), dptr, C.c_int, iptr, iptr, dptr, dptr,
                                         C.c_int, C.c_int, C.c_int, dptr]
    _lib = L
    return L


def _check(rc: int):
    if rc != XFK_OK:
        raise XfkError("xfk error %d: %s" % (rc, _lib.xfk_last_error().decode()))


def alloc_stats(reset: bool = False) -> dict:
    """Device allocations of the library since the last reset (diagnostics):
    hipMalloc / hipFree calls and their host milliseconds."""
    out = np.zeros(4)
    _check(load_library().xfk_alloc_stats(out.ctypes.data_as(dptr), int(reset)))
    return dict(n_malloc=int(out[0]), ms_malloc=float(out[1]), n_free=int(out[2]), ms_free=float(out[3]))


def cache_stats() -> dict:
    """The process-wide caches destroyed problems leave for the next one
    (xfk_cache_stats): device bytes, pinned host bytes, idle streams."""
    out = (C.c_longlong * 3)()
    _check(load_library().xfk_cache_stats(out))
    return dict(device_bytes=int(out[0]), pinned_bytes=int(out[1]), idle_streams=int(out[2]))


def release_cache():
    """Give the process-wide caches back to HIP (xfk_release_cache)."""
    _check(load_library().xfk_release_cache())


def forget_amg_hints():
    """Drop the AMG hints the last setup left for the next fresh problem of
    its size (xfk_amg_forget_hints): the next setup measures everything."""
    _check(load_library().xfk_amg_forget_hints())


def sort_elements(score, device: int = 0) -> np.ndarray:
    """FEASolver::SortElements' comb sort of element scores on the device
    (xfk_sort_elements): the permutation (position -> element)."""
    sc = np.ascontiguousarray(score, dtype=np.uint32)
    perm = np.empty(len(sc), dtype=np.int32)
    _check(load_library().xfk_sort_elements(len(sc), sc.ctypes.data_as(C.POINTER(C.c_uint)), device,
                                            perm.ctypes.data_as(iptr)))
    return perm


def device_count() -> int:
    return load_library().xfk_device_count()


class _Keep(list):
    def d(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self.append(a)
        return a.ctypes.data_as(dptr)

    def i(self, a):
        a = np.ascontiguousarray(a, dtype=np.int32)
        self.append(a)
        return a.ctypes.data_as(iptr)


def _make_desc(x, y, p, lbl, blocks, labels, lines, points, circuits, marker, e, pbc, precision, length_units,
               coords, relax, problem_type=0, ext=(0.0, 0.0, 0.0), ages=()):
    """xfk_problem_desc of plain arrays / dicts (see Static2DProblem); returns
    (desc, keep) where keep holds every buffer the descriptor points into."""
    keep = _Keep()
    nb = max(1, len(blocks))
    bl = (BlockDesc * nb)()
    for k, b in enumerate(blocks):
        o = bl[k]
        o.mu_x, o.mu_y = b.get("mu_x", 1.0), b.get("mu_y", 1.0)
        o.H_c, o.J_re, o.Cduct = b.get("H_c", 0.0), b.get("J_re", 0.0), b.get("Cduct", 0.0)
        o.LamFill, o.LamType = b.get("LamFill", 1.0), b.get("LamType", 0)
        n = len(b.get("B", ()))
        o.BHpoints = n
        if n:
            # (harmonic blocks may carry the complex curve: real parts here)
            o.B, o.H, o.slope = keep.d(b["B"]), keep.d(np.real(b["H"])), keep.d(np.real(b["slope"]))
    lb = (LabelDesc * max(1, len(labels)))()
    for k, l in enumerate(labels):
        lb[k].block, lb[k].in_circuit = l["block"], l.get("in_circuit", -1)
        lb[k].mag_dir, lb[k].is_wound = l.get("mag_dir", 0.0), int(l.get("is_wound", 0))
        lb[k].is_external = int(l.get("is_external", 0))
        f = l.get("mag_dir_fctn") or ""
        if f:
            fb = f.encode()
            keep.append(fb)
            lb[k].mag_dir_fctn = fb
    ln = (LineDesc * max(1, len(lines)))()
    for k, l in enumerate(lines):
        o = ln[k]
        o.format = l.get("format", 0)
        o.A0, o.A1, o.A2, o.phi = l.get("A0", 0.0), l.get("A1", 0.0), l.get("A2", 0.0), l.get("phi", 0.0)
        o.c0, o.c1 = l.get("c0", 0.0), l.get("c1", 0.0)
    pt = (PointDesc * max(1, len(points)))()
    for k, q in enumerate(points):
        pt[k].A_re, pt[k].A_im = q.get("A_re", 0.0), q.get("A_im", 0.0)
        pt[k].J_re, pt[k].J_im = q.get("J_re", 0.0), q.get("J_im", 0.0)
    ci = (CircuitDesc * max(1, len(circuits)))()
    for k, q in enumerate(circuits):
        ci[k].type, ci[k].amps_re, ci[k].dvolts_re = q.get("type", 0), q.get("amps_re", 0.0), q.get("dvolts_re", 0.0)
    D = ProblemDesc()
    x = np.asarray(x, dtype=np.float64)
    D.n_nodes = len(x)
    D.x, D.y = keep.d(x), keep.d(y)
    D.marker = keep.i(marker) if marker is not None else None
    p = np.asarray(p, dtype=np.int32).reshape(-1)
    D.n_elems = len(p) // 3
    D.p = keep.i(p)
    D.e = keep.i(np.asarray(e, dtype=np.int32).reshape(-1)) if e is not None else None
    D.lbl = keep.i(lbl)
    D.n_blocks, D.blocks = len(blocks), bl
    D.n_labels, D.labels = len(labels), lb
    D.n_lines, D.lines = len(lines), ln
    D.n_points, D.points = len(points), pt
    D.n_circs, D.circs = len(circuits), ci
    if pbc is not None and len(pbc):
        pb = np.asarray(pbc, dtype=np.int32).reshape(-1)
        D.n_pbc, D.pbc = len(pb) // 3, keep.i(pb)
    else:
        D.n_pbc, D.pbc = 0, None
    D.precision, D.length_units, D.coords, D.relax = precision, length_units, coords, relax
    D.problem_type = int(problem_type)
    D.ext_zo, D.ext_ro, D.ext_ri = ext
    # air-gap elements: dicts with format, ri, ro, total_arc_length, inner_shift,
    # outer_shift and the quadNode table qn / qw ((n_arc + 1) x 4 each)
    ag = (AgeDesc * max(1, len(ages)))()
    for k, a in enumerate(ages):
        o = ag[k]
        o.format, o.ri, o.ro = int(a.get("format", 0)), a["ri"], a["ro"]
        o.total_arc_length, o.inner_shift, o.outer_shift = a["total_arc_length"], a["inner_shift"], a["outer_shift"]
        qn = np.asarray(a["qn"], dtype=np.int32).reshape(-1, 4)
        o.n_arc = len(qn) - 1
        o.qn, o.qw = keep.i(qn), keep.d(np.asarray(a["qw"], dtype=np.float64).reshape(-1, 4))
    D.n_ages, D.ages = len(ages), ag
    keep.extend([bl, lb, ln, pt, ci, ag])
    return D, keep


def magdir_eval(fctn: str, p, x, y, length_units: int = 0, mag_dir: float = 0.0) -> np.ndarray:
    """Per-element magnetisation direction (degrees) of a label's MagDirFctn
    (xfk_magdir_eval; host only, no device needed).  Raises XfkError with the
    reference's message when the expression does not evaluate."""
    L = load_library()
    p = np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1))
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    n = len(p) // 3
    t = np.zeros(max(1, n))
    _check(L.xfk_magdir_eval(fctn.encode(), n, p.ctypes.data_as(iptr), x.ctypes.data_as(dptr),
                             y.ctypes.data_as(dptr), int(length_units), float(mag_dir), t.ctypes.data_as(dptr)))
    return t[:n]


def magdir_eval_labels(fctns, mag_dirs, p, lbl, x, y, length_units: int = 0, axisymmetric: bool = False,
                       repeats: bool = False) -> np.ndarray:
    """A whole problem's element loop of MagDirFctn (xfk_magdir_eval_labels):
    element i runs label lbl[i]'s function (None / "" for the label's MagDir)
    on one interpreter, in element order.  Host only."""
    L = load_library()
    p = np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1))
    lbl = np.ascontiguousarray(lbl, dtype=np.int32)
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    md = np.ascontiguousarray(mag_dirs, dtype=np.float64)
    fa = (C.c_char_p * max(1, len(fctns)))(*[(f or "").encode() for f in fctns])
    n = len(lbl)
    t = np.zeros(max(1, n))
    _check(L.xfk_magdir_eval_labels(len(fctns), fa, md.ctypes.data_as(dptr), n, p.ctypes.data_as(iptr),
                                    lbl.ctypes.data_as(iptr), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr),
                                    int(length_units), int(bool(axisymmetric)), int(bool(repeats)),
                                    t.ctypes.data_as(dptr)))
    return t[:n]


def lua_run(chunk: str) -> str:
    """Run a whole Lua chunk on a fresh native interpreter (xfk_lua_run) and
    return what it printed / wrote to the standard output.  Raises XfkError
    (code -2) for a Lua error, (-1) for a refused construct."""
    L = load_library()
    n = C.c_longlong(0)
    buf = C.create_string_buffer(1 << 16)
    rc = L.xfk_lua_run(chunk.encode(), buf, len(buf), C.byref(n))
    if n.value >= len(buf) and rc == 0:
        buf = C.create_string_buffer(n.value + 1)
        rc = L.xfk_lua_run(chunk.encode(), buf, len(buf), C.byref(n))
    _check(rc)
    return buf.raw[:n.value].decode("latin-1")


def age_element_matrix(ci: float, co: float, K: float, Ki: float) -> np.ndarray:
    """10 x 10 matrix of one air-gap arc element (host math of the C-ABI,
    cfemm/fsolver/static2d.cpp:209-263)."""
    L = load_library()
    out = np.zeros(100)
    rc = L.xfk_age_element_matrix(ci, co, K, Ki, out.ctypes.data_as(dptr))
    if rc != 0:
        raise XfkError("xfk_age_element_matrix failed (%d)" % rc)
    return out.reshape(10, 10)


class _MagPostProc:
    """Post-processing of a magnetostatic problem (the xfk_mag_ entry points):
    fpproc's element flux density, its block integrals that need no mask, the
    weighted stress tensor force and torque (types 18-23) over its mask, and
    its point values and contour integrals.
    The subclass provides _h, n_nodes, n_elems and n_labels.  A harmonic or a
    sharded problem is refused by the library with its cause."""

    # inttype -> name of the types answered (the others are 0)
    MAG_INTEGRALS = {0: "AJ", 1: "A", 2: "energy", 5: "area", 7: "current", 8: "B1", 9: "B2", 10: "volume",
                     11: "force_x", 12: "force_y", 15: "torque", 17: "coenergy", 24: "inertia", 25: "centroid"}

    def set_solution(self, A):
        """Post-process a given solution (one value per node as the .ans
        carries it: A, or the flux 2 pi r A on an axisymmetric problem)
        without solving (xfk_mag_set_solution)."""
        a = np.ascontiguousarray(A, dtype=np.float64)
        if a.shape != (self.n_nodes,):
            raise ValueError("expected one value per node (%d), got shape %s" % (self.n_nodes, a.shape))
        _check(_lib.xfk_mag_set_solution(self._h, a.ctypes.data_as(dptr)))

    def set_depth(self, depth: float):
        """[Depth] in the problem's length units; -1: the reference's default
        of 1 m, which also holds when this is never called (xfk_mag_set_depth)."""
        _check(_lib.xfk_mag_set_depth(self._h, float(depth)))

    def element_b(self) -> np.ndarray:
        """The flux density of every element, (n_elems, 2) (xfk_mag_element_b)."""
        B1 = np.zeros(self.n_elems)
        B2 = np.zeros(self.n_elems)
        _check(_lib.xfk_mag_element_b(self._h, B1.ctypes.data_as(dptr), B2.ctypes.data_as(dptr)))
        return np.stack([B1, B2], axis=1)

    def _mag_mask(self, selected_labels):
        m = np.zeros(max(1, self.n_labels), np.uint8)
        s = np.asarray(selected_labels)
        if s.dtype == np.bool_:
            m[:len(s)] = s
        elif s.size:
            m[s.astype(np.int64)] = 1
        return m, m.ctypes.data_as(C.POINTER(C.c_ubyte))

    def block_integrals(self, selected_labels) -> dict:
        """Every block integral over the elements of the selected labels
        (indices, or a boolean mask per label) from one pass over the mesh:
        the named types of MAG_INTEGRALS, and "raw", the complex values
        indexed by the reference's inttype (26 of them)."""
        keep, mp = self._mag_mask(selected_labels)
        o = np.zeros(52)
        _check(_lib.xfk_mag_block_integrals(self._h, mp, o.ctypes.data_as(dptr)))
        raw = o[0::2] + 1j * o[1::2]
        r = {name: (raw[t] if t == 25 else raw[t].real) for t, name in self.MAG_INTEGRALS.items()}
        r["raw"] = raw
        return r

    def block_integral(self, selected_labels, kind: int) -> complex:
        """One block integral in the reference's numbering (xfk_mag_block_integral)."""
        keep, mp = self._mag_mask(selected_labels)
        o = np.zeros(2)
        _check(_lib.xfk_mag_block_integral(self._h, mp, int(kind), o.ctypes.data_as(dptr)))
        return complex(o[0], o[1])

    def time_postproc(self, repeats: int = 5) -> dict:
        """Diagnostic: HIP-event times (ms, medians after a warm-up) of the
        element-B launch and of the block-integral launch with its sum, every
        label selected (xfk_mag_time)."""
        ms = np.zeros(2)
        _check(_lib.xfk_mag_time(self._h, int(repeats), ms.ctypes.data_as(dptr)))
        return dict(element_b=float(ms[0]), block_integrals=float(ms[1]))

    # -- a time-harmonic problem (the xfk_mag_ac_ entry points) --

    # inttype -> name of the types answered at Frequency != 0 (18-23 are 0)
    MAG_AC_INTEGRALS = {0: "AJ", 1: "A", 2: "energy", 3: "hysteresis_loss", 4: "resistive_loss", 5: "area",
                        6: "total_loss", 7: "current", 8: "B1", 9: "B2", 10: "volume", 11: "force_x", 12: "force_y",
                        13: "force_x_2f", 14: "force_y_2f", 15: "torque", 16: "torque_2f", 17: "coenergy",
                        24: "inertia", 25: "centroid"}

    def set_solution_complex(self, A):
        """Post-process a given harmonic solution (one complex value per node
        as the .ans carries it: A, or the flux 2 pi r A on an axisymmetric
        problem) without solving (xfk_mag_ac_set_solution)."""
        a = np.ascontiguousarray(A, dtype=np.complex128)
        if a.shape != (self.n_nodes,):
            raise ValueError("expected one value per node (%d), got shape %s" % (self.n_nodes, a.shape))
        _check(_lib.xfk_mag_ac_set_solution(self._h, a.view(np.float64).ctypes.data_as(dptr)))

    def element_b_complex(self) -> np.ndarray:
        """The complex flux density of every element, (n_elems, 2) (xfk_mag_ac_element_b)."""
        B1 = np.zeros(self.n_elems, np.complex128)
        B2 = np.zeros(self.n_elems, np.complex128)
        _check(_lib.xfk_mag_ac_element_b(self._h, B1.view(np.float64).ctypes.data_as(dptr),
                                         B2.view(np.float64).ctypes.data_as(dptr)))
        return np.stack([B1, B2], axis=1)

    def block_integrals_complex(self, selected_labels) -> dict:
        """Every block integral of a harmonic solution over the elements of
        the selected labels, from one pass over the mesh: the named types of
        MAG_AC_INTEGRALS as complex values, and "raw", indexed by the
        reference's inttype (26 of them; 18-23 are 0)."""
        keep, mp = self._mag_mask(selected_labels)
        o = np.zeros(52)
        _check(_lib.xfk_mag_ac_block_integrals(self._h, mp, o.ctypes.data_as(dptr)))
        raw = o[0::2] + 1j * o[1::2]
        r = {name: complex(raw[t]) for t, name in self.MAG_AC_INTEGRALS.items()}
        r["raw"] = raw
        return r

    def block_integral_complex(self, selected_labels, kind: int) -> complex:
        """One block integral of a harmonic solution in the reference's
        numbering (xfk_mag_ac_block_integral)."""
        keep, mp = self._mag_mask(selected_labels)
        o = np.zeros(2)
        _check(_lib.xfk_mag_ac_block_integral(self._h, mp, int(kind), o.ctypes.data_as(dptr)))
        return complex(o[0], o[1])

    def time_postproc_complex(self, repeats: int = 5) -> dict:
        """Diagnostic: HIP-event times (ms, medians after a warm-up) of the
        complex element-B launch and of the block-integral launch with its
        sum, every answerable label selected (xfk_mag_ac_time)."""
        ms = np.zeros(2)
        _check(_lib.xfk_mag_ac_time(self._h, int(repeats), ms.ctypes.data_as(dptr)))
        return dict(element_b=float(ms[0]), block_integrals=float(ms[1]))

    # -- the weighted stress tensor force and torque (block integrals 18-23) --

    def _mag_mask_args(self, selected_labels, max_area, block_not_air):
        sel, _ = self._mag_mask(selected_labels)
        area = None
        if max_area is not None:
            area = np.ascontiguousarray(max_area, dtype=np.float64)
            if area.shape != (self.n_labels,):
                raise ValueError("expected one MaxArea per label (%d), got shape %s" % (self.n_labels, area.shape))
        notair = None
        if block_not_air is not None:
            notair = np.ascontiguousarray(np.asarray(block_not_air) != 0, dtype=np.uint8)
            if notair.shape != (self.n_blocks,):
                raise ValueError("expected one flag per block (%d), got shape %s" % (self.n_blocks, notair.shape))
        return sel, area, notair

    def _mag_mask_defaults(self):
        """(max_area, block_not_air) a make_mask without them takes: nothing
        for an in-memory problem; a file-solved one knows its .fem's."""
        return None, None

    def _mag_mask_fill(self, max_area, block_not_air):
        """each argument left None takes its default"""
        if max_area is None or block_not_air is None:
            a, b = self._mag_mask_defaults()
            max_area = a if max_area is None else max_area
            block_not_air = b if block_not_air is None else block_not_air
        return max_area, block_not_air

    def mask_info(self) -> dict:
        """Whether the problem holds a mask, and the last make_mask's PCG
        iterations and times in ms (xfk_mag_mask_info)."""
        o = np.zeros(9)
        _check(_lib.xfk_mag_mask_info(self._h, o.ctypes.data_as(dptr)))
        return dict(ready=bool(o[0]), cg_iters=int(o[1]),
                    times=dict(create=o[2], fixed_values=o[3], symbolic=o[4], assemble=o[5], amg_setup=o[6],
                               solve=o[7], total=o[8]))

    def make_mask(self, selected_labels, max_area=None, block_not_air=None) -> dict:
        """FPProc::MakeMask for the selected labels (indices or a boolean mask
        per label); max_area: the labels' MaxArea (None: the element areas
        weight the Laplacian); block_not_air: per block, non-zero where a
        hysteresis angle makes it other than air.  Returns W (the solved nodal
        values), msk (W > 0.5 as 0 / 1), cg_iters and times (ms)."""
        ubp = C.POINTER(C.c_ubyte)
        max_area, block_not_air = self._mag_mask_fill(max_area, block_not_air)
        sel, area, notair = self._mag_mask_args(selected_labels, max_area, block_not_air)
        self._mag_mask_key = None
        _check(_lib.xfk_mag_make_mask(self._h, sel.ctypes.data_as(ubp),
                                      None if area is None else area.ctypes.data_as(dptr),
                                      None if notair is None else notair.ctypes.data_as(ubp)))
        self._mag_mask_key = tuple(None if a is None else a.tobytes() for a in (sel, area, notair))
        W = np.zeros(self.n_nodes)
        msk = np.zeros(self.n_nodes)
        _check(_lib.xfk_mag_get_mask(self._h, W.ctypes.data_as(dptr), msk.ctypes.data_as(dptr)))
        info = self.mask_info()
        return dict(W=W, msk=msk, cg_iters=info["cg_iters"], times=info["times"])

    def mask_csr(self):
        """Diagnostic: the assembled system of the last mask solve, as csr()."""
        h = C.c_void_p()
        _check(_lib.xfk_mag_mask_problem(self._h, C.byref(h)))
        nnz = _lib.xfk_get_nnz(h)
        rp = np.zeros(self.n_nodes + 1, np.int32)
        col = np.zeros(nnz, np.int32)
        val = np.zeros(nnz)
        b = np.zeros(self.n_nodes)
        _check(_lib.xfk_get_csr(h, rp.ctypes.data_as(iptr), col.ctypes.data_as(iptr), val.ctypes.data_as(dptr),
                                b.ctypes.data_as(dptr)))
        return rp, col, val, b

    def weighted_stress(self, selected_labels, max_area=None, block_not_air=None) -> dict:
        """The weighted stress tensor force (N) and torque about the origin
        (N m) on the selection with their "2x" parts: block integrals 18-23,
        the mask made first unless the problem holds the one of these very
        arguments."""
        max_area, block_not_air = self._mag_mask_fill(max_area, block_not_air)
        key = tuple(None if a is None else a.tobytes()
                    for a in self._mag_mask_args(selected_labels, max_area, block_not_air))
        if getattr(self, "_mag_mask_key", None) != key or not self.mask_info()["ready"]:
            self.make_mask(selected_labels, max_area, block_not_air)
        # (one type at a time: these are answered whatever the selected blocks are)
        z = [self.block_integral(selected_labels, t).real for t in range(18, 24)]
        return dict(force=np.array([z[0], z[1]]), force_2x=np.array([z[2], z[3]]), torque=z[4], torque_2x=z[5])

    def time_stress(self, repeats: int = 5) -> float:
        """Diagnostic: HIP-event ms (median) of the integral launch of types 18-23."""
        ms = C.c_double()
        _check(_lib.xfk_mag_stress_time(self._h, int(repeats), C.byref(ms)))
        return ms.value

    # -- point values and contour integrals (GetNodalB, GetPointValues, LineIntegral) --

    # the values of xfk_mag_point_values per point, in its order
    MAG_POINT_NAMES = ("A", "B1", "B2", "mu1", "mu2", "H1", "H2", "Js", "c", "E", "Hc_re", "Hc_im", "ff")

    def corner_b(self) -> np.ndarray:
        """GetNodalB of every element, (n_elems, 3, 2): (b1, b2) of its
        corners (xfk_mag_corner_b)."""
        b = np.zeros(6 * max(1, self.n_elems))
        _check(_lib.xfk_mag_corner_b(self._h, b.ctypes.data_as(dptr)))
        return b[:6 * self.n_elems].reshape(-1, 3, 2)

    @staticmethod
    def _mag_points(x, y):
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        if x.shape != y.shape or x.ndim != 1:
            raise ValueError("x and y must be one-dimensional and of one length")
        return x, y

    def _mag_point_dict(self, el, o):
        r = {"elem": el, "raw": o}
        for k, name in enumerate(self.MAG_POINT_NAMES):
            r[name] = o[:, k].copy()
        r["Hc"] = r.pop("Hc_re") + 1j * r.pop("Hc_im")
        # 0 at Frequency 0; the keys of mo_getpointvalues
        for name in ("Je", "Ph", "Pe"):
            r[name] = np.zeros(len(el))
        return r

    def point_values(self, x, y, smooth: bool = True) -> dict:
        """GetPointValues at the points (x, y), in the problem's length units:
        elem (the lowest-numbered containing element, -1 outside the mesh: its
        values are NaN), raw (n, 13) and the reference's point-value fields by
        name (MAG_POINT_NAMES, Hc complex; Je, Ph and Pe are 0 at Frequency 0)."""
        x, y = self._mag_points(x, y)
        n = len(x)
        el = np.zeros(max(1, n), np.int32)
        o = np.zeros((max(1, n), 13))
        _check(_lib.xfk_mag_point_values(self._h, n, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(bool(smooth)),
                                         el.ctypes.data_as(iptr), o.ctypes.data_as(dptr)))
        return self._mag_point_dict(el[:n], o[:n])

    def point_values_at(self, x, y, elem, smooth: bool = True) -> dict:
        """point_values with the element of every point given (xfk_mag_point_values_at)."""
        x, y = self._mag_points(x, y)
        el = np.ascontiguousarray(np.atleast_1d(elem), dtype=np.int32)
        n = len(x)
        o = np.zeros((max(1, n), 13))
        _check(_lib.xfk_mag_point_values_at(self._h, n, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr),
                                            el.ctypes.data_as(iptr), int(bool(smooth)), o.ctypes.data_as(dptr)))
        return self._mag_point_dict(el[:n], o[:n])

    @staticmethod
    def _mag_contours(contours):
        xy = [_PotentialPostProc._contour_xy(c) for c in contours]
        ptr = np.zeros(len(xy) + 1, np.int32)
        ptr[1:] = np.cumsum([len(x) for x, _ in xy])
        x = np.ascontiguousarray(np.concatenate([x for x, _ in xy] + [np.zeros(1)]))
        y = np.ascontiguousarray(np.concatenate([y for _, y in xy] + [np.zeros(1)]))
        return len(xy), ptr, x, y

    def line_integrals(self, contours, kind: int, smooth: bool = True, points: int = 400) -> dict:
        """fpproc's LineIntegral of type `kind` (0 B.n, 1 H.t, 2 length, 3
        stress tensor force, 4 torque, 5 (B.n)^2) over a batch of contours:
        each a Contour, a sequence of (x, y) or of complex points, in the
        problem's length units.  raw: (n, 2), the two results per contour;
        missed: per contour the samples no element contains (they add
        nothing).  Every contour's result has the bits it has when integrated
        alone.  Type 4 is 0 on an axisymmetric problem."""
        n, ptr, x, y = self._mag_contours(contours)
        o = np.zeros((max(1, n), 2))
        missed = np.zeros(max(1, n), np.int32)
        _check(_lib.xfk_mag_line_integrals(self._h, n, ptr.ctypes.data_as(iptr), x.ctypes.data_as(dptr),
                                           y.ctypes.data_as(dptr), int(kind), int(bool(smooth)), int(points),
                                           o.ctypes.data_as(dptr), missed.ctypes.data_as(iptr)))
        return {"raw": o[:n], "missed": missed[:n]}

    def line_integral(self, contour, kind: int, smooth: bool = True, points: int = 400) -> complex:
        """One contour's LineIntegral of type `kind`: the two results as a
        complex number (xfk_mag_line_integral)."""
        x, y = _PotentialPostProc._contour_xy(contour)
        o = np.zeros(2)
        _check(_lib.xfk_mag_line_integral(self._h, len(x), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(kind),
                                          int(bool(smooth)), int(points), o.ctypes.data_as(dptr), None))
        return complex(o[0], o[1])

    def contour_samples(self, contour, kind: int, points: int = 400) -> dict:
        """Diagnostic: the samples of one contour as the kernel makes them, xy
        (n, 2) and the element each took, -1 for none (xfk_mag_contour_samples)."""
        x, y = _PotentialPostProc._contour_xy(contour)
        ns = max(0, len(x) - 1) * (int(points) if points > 0 else 400)
        xy = np.zeros((max(1, ns), 2))
        el = np.zeros(max(1, ns), np.int32)
        _check(_lib.xfk_mag_contour_samples(self._h, len(x), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(kind),
                                            int(points), xy.ctypes.data_as(dptr), el.ctypes.data_as(iptr)))
        return {"xy": xy[:ns], "elem": el[:ns]}

    def time_points(self, x, y, repeats: int = 5) -> dict:
        """Diagnostic: HIP-event ms (medians after a warm-up) of the corner
        kernel, the cell grid and the point kernel on these points with
        smoothing off and on (xfk_mag_point_time)."""
        x, y = self._mag_points(x, y)
        ms = np.zeros(4)
        _check(_lib.xfk_mag_point_time(self._h, len(x), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(repeats),
                                       ms.ctypes.data_as(dptr)))
        return dict(corner=float(ms[0]), grid=float(ms[1]), points=float(ms[2]), points_smooth=float(ms[3]))

    def time_contours(self, contours, kind: int, smooth: bool = True, points: int = 400, repeats: int = 5) -> float:
        """Diagnostic: HIP-event ms (median) of the contour kernel and its sums
        over the batch (xfk_mag_contour_time)."""
        n, ptr, x, y = self._mag_contours(contours)
        ms = C.c_double()
        _check(_lib.xfk_mag_contour_time(self._h, n, ptr.ctypes.data_as(iptr), x.ctypes.data_as(dptr),
                                         y.ctypes.data_as(dptr), int(kind), int(bool(smooth)), int(points),
                                         int(repeats), C.byref(ms)))
        return ms.value



class Static2DProblem(_MagPostProc):
    """One device-resident static 2-D magnetostatic problem (FSolver::Static2D).

    Arrays follow the reference's in-memory state after FSolver::LoadMesh and
    LoadProblemFile (cm coordinates, 0-based indices, -1 for "none")."""

    def __init__(self, *, x, y, p, lbl, blocks: Sequence[dict], labels: Sequence[dict],
                 lines: Sequence[dict] = (), points: Sequence[dict] = (), circuits: Sequence[dict] = (),
                 marker=None, e=None, pbc=None, precision=1e-8, length_units=0, coords=0, relax=1.0,
                 device=0, comm: Optional["Comm"] = None, precond: str = "amg", amg_sweeps: Optional[int] = None,
                 amg_theta: Optional[float] = None, frequency: float = 0.0, amg_omega: Optional[float] = None,
                 amg_replicate: Optional[int] = None, amg_reuse: Optional[bool] = None, problem_type: int = 0,
                 ext_zo: float = 0.0, ext_ro: float = 0.0, ext_ri: float = 0.0, amg_dense: Optional[int] = None,
                 ages: Sequence[dict] = (), ac_solver: int = 0, amg_fold: Optional[bool] = None,
                 amg_col16: Optional[bool] = None, amg_wlevel: Optional[int] = None,
                 amg_f32: Optional[bool] = None, newton_inexact: Optional[bool] = None):
        """ac_solver: [ACSolver], read by the harmonic solvers only (ignored here).
        newton_inexact: nonlinear passes before the last solved to a forcing
        tolerance (default on; False: every pass to Precision, as the
        reference; XFK_OPT_NEWTON_INEXACT).
        amg_fold: folded V(1,1) levels (default on; False: the plain cycle).
        amg_col16: 16-bit tile column offsets on level 0 (default on; False:
        int columns; the same bits either way).
        amg_wlevel: the folded coarse level that runs a W-cycle (default: the
        level above the last V-cycle level; -1: a plain V-cycle).
        amg_f32: f32 values for the V-cycle's level-0 transfers R and P~
        (default on; False: f64; the sweeps and the PCG SpMV stay f64).
        comm: shard the mesh by row blocks over this communicator (every rank
        passes the same global problem; solve() and solution() are collective).
        precond: "amg" (smoothed-aggregation V-cycle, default) or "jacobi".
        problem_type: XFK_PLANAR (Static2D) or XFK_AXISYMMETRIC
        (StaticAxisymmetric: x is r, y is z; solution() is the flux 2 pi r A)."""
        if frequency:
            raise XfkError("frequency != 0: use Harmonic2DProblem")
        L = load_library()
        D, keep = _make_desc(x, y, p, lbl, blocks, labels, lines, points, circuits, marker, e, pbc, precision,
                             length_units, coords, relax, problem_type, (ext_zo, ext_ro, ext_ri), ages)
        self._keep = keep
        self.n_nodes = D.n_nodes
        self.n_elems = D.n_elems
        self.n_circs = len(circuits)
        self.n_labels = len(labels)
        self.n_blocks = len(blocks)
        h = C.c_void_p()
        self.comm = comm
        if comm is None:
            _check(L.xfk_problem_create(C.byref(D), device, C.byref(h)))
        else:
            _check(L.xfk_problem_create_dist(C.byref(D), device, comm._h, C.byref(h)))
        self._h = h
        self.set_option(XFK_OPT_PRECOND, PRECONDS[precond])
        if amg_sweeps is not None:
            self.set_option(XFK_OPT_AMG_SWEEPS, amg_sweeps)
        if amg_theta is not None:
            self.set_option(XFK_OPT_AMG_THETA, amg_theta)
        if amg_omega is not None:
            self.set_option(XFK_OPT_AMG_OMEGA, amg_omega)
        if amg_replicate is not None:
            self.set_option(XFK_OPT_AMG_REPLICATE, amg_replicate)
        if amg_reuse is not None:
            self.set_option(XFK_OPT_AMG_REUSE, int(bool(amg_reuse)))
        if amg_dense is not None:
            self.set_option(XFK_OPT_AMG_DENSE, amg_dense)
        if amg_fold is not None:
            self.set_option(XFK_OPT_AMG_FOLD, int(bool(amg_fold)))
        if amg_col16 is not None:
            self.set_option(XFK_OPT_AMG_COL16, int(bool(amg_col16)))
        if amg_f32 is not None:
            self.set_option(XFK_OPT_AMG_F32, int(bool(amg_f32)))
        if amg_wlevel is not None:
            self.set_option(XFK_OPT_AMG_WLEVEL, int(amg_wlevel))
        if newton_inexact is not None:
            self.set_option(XFK_OPT_NEWTON_INEXACT, int(bool(newton_inexact)))
        self.n_rows = self.dist_info()["n_own"] if comm is not None else self.n_nodes
        self.result: Optional[Result] = None

    def set_option(self, option: int, value: float):
        _check(_lib.xfk_set_option(self._h, option, float(value)))

    def memory(self) -> dict:
        """Device memory of this problem (xfk_problem_memory): arena chunk
        bytes and count, bytes carved and live, bytes kept for reuse."""
        out = (C.c_longlong * 4)()
        _check(_lib.xfk_problem_memory(self._h, out))
        return dict(chunk_bytes=int(out[0]), chunks=int(out[1]), live_bytes=int(out[2]), reuse_bytes=int(out[3]))

    def dist_info(self) -> dict:
        info = DistInfo()
        _check(_lib.xfk_dist_get_info(self._h, C.byref(info)))
        return info.as_dict()

    def close(self):
        if getattr(self, "_h", None):
            load_library().xfk_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, rebuild_symbolic: bool = False, time_spmv: bool = False, time_tail: bool = False) -> dict:
        r = Result()
        flags = ((XFK_REBUILD_SYMBOLIC if rebuild_symbolic else 0) | (XFK_TIME_SPMV if time_spmv else 0) |
                 (XFK_TIME_TAIL if time_tail else 0))
        _check(_lib.xfk_static2d(self._h, flags, C.byref(r)))
        self.result = r
        return r.as_dict()

    def solution(self) -> np.ndarray:
        A = np.zeros(self.n_nodes)
        _check(_lib.xfk_get_solution(self._h, A.ctypes.data_as(dptr)))
        return A

    def circuits(self):
        n = self.n_circs
        cc = np.zeros(max(1, n), np.int32)
        J = np.zeros(max(1, n))
        dV = np.zeros(max(1, n))
        _check(_lib.xfk_get_circuits(self._h, cc.ctypes.data_as(iptr), J.ctypes.data_as(dptr),
                                     dV.ctypes.data_as(dptr)))
        return cc[:n], J[:n], dV[:n]

    def assemble_at(self, V_list=()):
        """The system of Newton pass len(V_list) without solving
        (xfk_static2d_assemble_at): the iteration-0 system from V = 0, then one
        pass per iterate of V_list, each reading the permeability state the
        pass before wrote.  The iterates are in the solver's own unit (planar:
        solution() / c with c = 4e-5 pi); csr() and element_state() then show
        the last pass."""
        V = np.ascontiguousarray(np.asarray(V_list, dtype=np.float64).reshape(len(V_list), -1 if len(V_list) else 0))
        if len(V) and V.shape[1] != self.n_nodes:
            raise XfkError("every iterate needs n_nodes values")
        _check(_lib.xfk_static2d_assemble_at(self._h, len(V), V.ctypes.data_as(dptr) if len(V) else None))

    def element_state(self):
        """(mu1, mu2) per element, the caller's element order: the permeability
        state the last pass wrote (xfk_get_element_state; nonlinear problems)."""
        mu1 = np.zeros(self.n_elems)
        mu2 = np.zeros(self.n_elems)
        _check(_lib.xfk_get_element_state(self._h, mu1.ctypes.data_as(dptr), mu2.ctypes.data_as(dptr)))
        return mu1, mu2

    def spmv_col_bytes(self) -> float:
        """Column-index bytes per nonzero of the last solve's PCG SpMV (2: the
        AMG's 16-bit tile offsets, 4: int columns)."""
        return float(_lib.xfk_spmv_col_bytes(self._h))

    def csr(self):
        """This rank's rows (all rows unless sharded; sharded columns are local ids)."""
        nnz = _lib.xfk_get_nnz(self._h)
        rp = np.zeros(self.n_rows + 1, np.int32)
        col = np.zeros(nnz, np.int32)
        val = np.zeros(nnz)
        b = np.zeros(self.n_rows)
        _check(_lib.xfk_get_csr(self._h, rp.ctypes.data_as(iptr), col.ctypes.data_as(iptr),
                                val.ctypes.data_as(dptr), b.ctypes.data_as(dptr)))
        return rp, col, val, b

    def pcg_time(self, iters: int = 50):
        ms_spmv = C.c_double()
        ms_iter = C.c_double()
        _check(_lib.xfk_pcg_time(self._h, iters, C.byref(ms_spmv), C.byref(ms_iter)))
        return ms_spmv.value, ms_iter.value

    def phase_profile(self, iters: int = 10, setup: bool = True):
        """Per-phase HIP-event profile (xfk_phase_profile): list of dicts
        name, calls, ms_total, us_per_call, bytes_per_call."""
        cap = 256
        buf = (Phase * cap)()
        n = C.c_int()
        _check(_lib.xfk_phase_profile(self._h, iters, XFK_PROFILE_SETUP if setup else 0, C.cast(buf, C.c_void_p),
                                      cap, C.byref(n)))
        out = []
        for k in range(n.value):
            ph = buf[k]
            out.append(dict(name=ph.name.decode(), calls=ph.calls, ms_total=ph.ms_total,
                            us_per_call=1e3 * ph.ms_total / max(1, ph.calls), bytes_per_call=ph.bytes_per_call))
        return out


class Contour:
    """The contour of the reference's post-processors, built on the host as
    PostProcessor builds it: a list of (x, y) in the problem's length units."""

    def __init__(self, points=()):
        self.points = []
        for x, y in points:
            self.add(x, y)

    def __len__(self):
        return len(self.points)

    def add(self, x, y):
        """addContourPoint (PostProcessor.cpp:167-171): a point equal to the last is dropped."""
        z = (float(x), float(y))
        if not self.points or z != self.points[-1]:
            self.points.append(z)
        return self

    def clear(self):
        """clearContour."""
        self.points = []
        return self

    def add_point_from_node(self, geometry, x, y):
        """addContourPointFromNode (PostProcessor.cpp:173-298) over the input
        geometry of a solution file (pproc.EPProc.geometry(): points (n, 2),
        segments (n, 2), arcs (n, 2) with arc_length and arc_maxside in
        degrees): the input point closest to (x, y) is added; when it and the
        last contour point are the two ends of an arc segment, the arc is
        followed in ceil(ArcLength / MaxSideLength) steps, the last of which is
        the input point itself."""
        P = np.asarray(geometry["points"], float).reshape(-1, 2)
        if len(P) == 0:
            return self
        pi = 3.141592653589793238462643383

        def closest(px, py):
            return int(np.argmin(np.sqrt((px - P[:, 0]) ** 2 + (py - P[:, 1]) ** 2)))

        def circle(k):
            a0, a1 = complex(*P[geometry["arcs"][k][0]]), complex(*P[geometry["arcs"][k][1]])
            d = abs(a1 - a0)
            t = (a1 - a0) / d
            tta = geometry["arc_length"][k] * pi / 180.
            R = d / (2. * math.sin(tta / 2.))
            return a0 + (d / 2. + 1j * math.sqrt(R * R - d * d / 4.)) * t, R

        def dist_arc(p, k):
            c, R = circle(k)
            d = abs(p - c)
            if d == 0:
                return R
            a0, a1 = complex(*P[geometry["arcs"][k][0]]), complex(*P[geometry["arcs"][k][1]])
            t = (p - c) / d
            z = cmath.phase(t / (a0 - c)) * 180 / pi
            if 0 < z < geometry["arc_length"][k]:
                return abs(p - c - R * t)
            return min(abs(p - a0), abs(p - a1))

        def dist_seg(k):
            (x0, y0), (x1, y1) = P[geometry["segments"][k][0]], P[geometry["segments"][k][1]]
            t = ((x - x0) * (x1 - x0) + (y - y0) * (y1 - y0)) / ((x1 - x0) ** 2 + (y1 - y0) ** 2)
            t = min(1., max(0., t))
            return math.hypot(x - (x0 + t * (x1 - x0)), y - (y0 + t * (y1 - y0)))

        x, y = float(x), float(y)
        n0 = closest(x, y)
        z = complex(*P[n0])
        if not self.points:
            self.points.append((z.real, z.imag))
            return self
        last = complex(*self.points[-1])
        if last == z:
            return self
        n1 = closest(last.real, last.imag)
        line, arc, rev, d1 = -1, -1, False, 1.e08
        if abs(complex(*P[n1]) - last) < 1.e-08:
            for k, (a, b) in enumerate(np.asarray(geometry["segments"], int).reshape(-1, 2)):
                if (a, b) in ((n1, n0), (n0, n1)):
                    d2 = dist_seg(k)
                    if d2 < d1:
                        line, d1 = k, d2
            for k, (a, b) in enumerate(np.asarray(geometry["arcs"], int).reshape(-1, 2)):
                for r in (True, False):
                    if (a, b) == ((n1, n0) if r else (n0, n1)):
                        d2 = dist_arc(complex(x, y), k)
                        if d2 < d1:
                            arc, line, rev, d1 = k, -1, r, d2

        def behind(q):
            return len(self.points) > 1 and abs(complex(*self.points[-2]) - q) < 1.e-08

        if line < 0 and arc < 0:
            self.points.append((z.real, z.imag))
        if line >= 0:
            if behind(z):
                return self
            self.points.append((z.real, z.imag))
        if arc >= 0:
            c, _ = circle(arc)
            n = int(math.ceil(geometry["arc_length"][arc] / geometry["arc_maxside"][arc]))
            th = geometry["arc_length"][arc] * pi / (180. * float(n))
            rot = complex(math.cos(th), math.sin(th) if rev else -math.sin(th))
            w = last
            for i in range(n):
                w = (w - c) * rot + c
                if i == n - 1:
                    w = z
                if behind(w):
                    return self
                self.points.append((w.real, w.imag))
        return self

    def bend(self, angle, step=1.0):
        """bendContour (PostProcessor.cpp:772-820): the last segment becomes an
        arc of `angle` degrees in steps of `step` (0: 1).  An angle of 0 or
        outside +-180, or a contour of fewer than two points, changes nothing."""
        pi = 3.141592653589793238462643383
        if angle == 0:
            return self
        if step == 0:
            step = 1
        k = len(self.points) - 1
        if k < 1:
            return self
        if angle < -180. or angle > 180.:
            return self
        n = int(math.ceil(abs(angle / step)))
        tta = angle * pi / 180.
        dtta = tta / float(n)
        a1 = self.points.pop(k)
        a0 = self.points[k - 1]
        dr, di = a1[0] - a0[0], a1[1] - a0[1]
        if dr == 0 and di == 0:
            d = 0.
        elif abs(dr) > abs(di):
            d = abs(dr) * math.sqrt(1. + (di / dr) * (di / dr))
        else:
            d = abs(di) * math.sqrt(1. + (dr / di) * (dr / di))
        R = d / (2. * math.sin(abs(tta / 2.)))
        ph = (pi - tta) / 2. if tta > 0 else (-1. * (pi + tta)) / 2.
        er, ei = math.cos(ph), math.sin(ph)
        sr, si = (R / d) * dr, (R / d) * di
        cr, ci = a0[0] + (sr * er - si * ei), a0[1] + (sr * ei + si * er)
        vr, vi = a0[0] - cr, a0[1] - ci
        for k in range(1, n + 1):
            er, ei = math.cos(float(k) * dtta), math.sin(float(k) * dtta)
            self.points.append((cr + (vr * er - vi * ei), ci + (vr * ei + vi * er)))
        return self


class _PotentialPostProc:
    """Post-processing shared by ElectrostaticProblem and HeatFlowProblem (the
    reference's epproc / hpproc on the device, xfk_pot_*).  _POINT_NAMES: the
    names of the reference's point-value struct over the 8 values per point."""

    _FIELD_NAMES = ("D", "E")
    _INTEGRAL_NAMES = ("energy", "area", "volume", "D", "E")

    def set_solution(self, V):
        """Load a nodal solution (one value per node) and mark the problem solved."""
        v = np.ascontiguousarray(V, dtype=np.float64)
        if v.shape != (self.n_nodes,):
            raise ValueError("expected one value per node (%d), got shape %s" % (self.n_nodes, v.shape))
        _check(_lib.xfk_pot_set_solution(self._h, v.ctypes.data_as(dptr)))

    def qmarks(self) -> np.ndarray:
        """The mark of every node as the reference's L.Q holds it: a conductor's
        index, else -1 on a fixed node, else -2."""
        Q = np.zeros(self.n_nodes, np.int32)
        _check(_lib.xfk_pot_get_qmarks(self._h, Q.ctypes.data_as(iptr)))
        return Q

    def set_qmarks(self, Q):
        """The Q column of a solution file in place of the descriptor's marks,
        before set_solution.  The problem then counts as opened from a file:
        solve() is refused from here on (xfk_pot_set_qmarks)."""
        q = np.ascontiguousarray(Q, dtype=np.int32)
        if q.shape != (self.n_nodes,):
            raise ValueError("expected one mark per node (%d), got shape %s" % (self.n_nodes, q.shape))
        _check(_lib.xfk_pot_set_qmarks(self._h, q.ctypes.data_as(iptr)))

    def plot_bounds(self) -> np.ndarray:
        """d_PlotBounds of the reference's OpenDocument, (3, 2): min and max of
        the potential over the nodes, of |D| (|F|) and of |E| (|G|) over the
        elements that are not external, with the reference's starting
        elements (xfk_pot_plot_bounds)."""
        o = np.zeros(6)
        _check(_lib.xfk_pot_plot_bounds(self._h, o.ctypes.data_as(dptr)))
        return o.reshape(3, 2)

    def element_fields(self) -> dict:
        """Per element D and E (F and G for heat flow), (n_elems, 2) each."""
        D = np.zeros((self.n_elems, 2))
        E = np.zeros((self.n_elems, 2))
        _check(_lib.xfk_pot_element_fields(self._h, D.ctypes.data_as(dptr), E.ctypes.data_as(dptr)))
        return {self._FIELD_NAMES[0]: D, self._FIELD_NAMES[1]: E}

    def corner_fields(self) -> np.ndarray:
        """The smoothed D (F) at the corners of every element, (n_elems, 3, 2)."""
        d = np.zeros((self.n_elems, 3, 2))
        _check(_lib.xfk_pot_corner_fields(self._h, d.ctypes.data_as(dptr)))
        return d

    def corner_branches(self) -> np.ndarray:
        """Diagnostic: which case of the smoothing each corner took, (n_elems,
        3): 0 the fit, 1-5 the reference's punts in its order, 6 a singular fit."""
        b = np.zeros((self.n_elems, 3), np.uint8)
        _check(_lib.xfk_pot_corner_branches(self._h, b.ctypes.data_as(C.POINTER(C.c_ubyte))))
        return b

    def grid_info(self) -> dict:
        """Diagnostic: the cell grid of the point search (xfk_pot_grid_info)."""
        o = np.zeros(8)
        _check(_lib.xfk_pot_grid_info(self._h, o.ctypes.data_as(dptr)))
        return dict(x0=o[0], y0=o[1], cells_per_x=o[2], cells_per_y=o[3], nx=int(o[4]), ny=int(o[5]),
                    oversize=int(o[6]), entries=int(o[7]))

    def time_postproc(self, x, y, repeats: int = 5) -> dict:
        """Diagnostic: HIP-event times (ms, medians) of the post-processing
        launches and the mean triangle tests per point (xfk_pot_time)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        ms = np.zeros(7)
        tests = C.c_double()
        _check(_lib.xfk_pot_time(self._h, len(x), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(repeats),
                                 ms.ctypes.data_as(dptr), C.byref(tests)))
        names = ("mesh_tables_host", "cell_grid", "element_fields", "corner_fields", "block_integrals",
                 "points", "points_smooth")
        r = dict(zip(names, ms.tolist()))
        r["tests_per_point"] = tests.value
        return r

    def _mask(self, selected_labels):
        if selected_labels is None:
            return None, None
        m = np.zeros(max(1, self.n_labels), np.uint8)
        s = np.asarray(selected_labels)
        if s.dtype == np.bool_:
            m[:len(s)] = s
        else:
            m[s.astype(np.int64)] = 1
        return m, m.ctypes.data_as(C.POINTER(C.c_ubyte))

    def block_integrals(self, selected_labels) -> dict:
        """The reference's block integrals 0-4 over the elements of the selected
        labels (indices, or a boolean mask per label)."""
        keep, mp = self._mask(selected_labels)
        o = np.zeros(7)
        _check(_lib.xfk_pot_block_integrals(self._h, mp, o.ctypes.data_as(dptr)))
        n = self._INTEGRAL_NAMES
        return {n[0]: o[0], n[1]: o[1], n[2]: o[2], n[3]: o[3:5].copy(), n[4]: o[5:7].copy(), "raw": o}

    def block_integrals_ordered(self, selected_labels) -> np.ndarray:
        """The seven sums of block_integrals taken element by element, in the
        reference's order of summation (xfk_pot_block_integrals_ordered)."""
        keep, mp = self._mask(selected_labels)
        o = np.zeros(7)
        _check(_lib.xfk_pot_block_integrals_ordered(self._h, mp, o.ctypes.data_as(dptr)))
        return o

    def point_values_at(self, x, y, elem, smooth: bool = False) -> np.ndarray:
        """The 8 values per point with the element of every point given, (n, 8)
        (xfk_pot_point_values_at)."""
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        el = np.ascontiguousarray(np.atleast_1d(elem), dtype=np.int32)
        o = np.zeros((max(1, len(x)), 8))
        _check(_lib.xfk_pot_point_values_at(self._h, len(x), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr),
                                            el.ctypes.data_as(iptr), int(bool(smooth)), o.ctypes.data_as(dptr)))
        return o[:len(x)]

    def block_integral(self, selected_labels, kind: int) -> complex:
        """One block integral in the reference's numbering: 0-4, and on an
        electrostatic problem holding a mask made for this selection
        (make_mask) 5 and 6, the weighted stress tensor force and torque."""
        keep, mp = self._mask(selected_labels)
        o = np.zeros(2)
        _check(_lib.xfk_pot_block_integral(self._h, mp, int(kind), o.ctypes.data_as(dptr)))
        return complex(o[0], o[1])

    def point_values(self, x, y, smooth: bool = False) -> dict:
        """getPointValues at the points (x, y), in the problem's length units:
        elem (the lowest-numbered containing element, -1 outside the mesh:
        its values are NaN) and the reference's point-value fields."""
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        if x.shape != y.shape or x.ndim != 1:
            raise ValueError("x and y must be one-dimensional and of one length")
        n = len(x)
        el = np.zeros(max(1, n), np.int32)
        o = np.zeros((max(1, n), 8))
        _check(_lib.xfk_pot_point_values(self._h, n, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(bool(smooth)),
                                         el.ctypes.data_as(iptr), o.ctypes.data_as(dptr)))
        o = o[:n]
        r = {"elem": el[:n], "raw": o}
        for name, cols in self._POINT_NAMES:
            r[name] = o[:, cols].copy()
        return r

    @staticmethod
    def _contour_xy(contour):
        pts = contour.points if isinstance(contour, Contour) else contour
        a = np.asarray(pts)
        if a.ndim == 1 and np.iscomplexobj(a):
            a = np.stack([a.real, a.imag], axis=1)
        a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
        return np.ascontiguousarray(a[:, 0]), np.ascontiguousarray(a[:, 1])

    def line_integrals(self, contours, kind: int, smooth: bool = True, points: int = 400) -> dict:
        """The reference's lineIntegral of type `kind` (its numbering) over a
        batch of contours: each a Contour, a sequence of (x, y) or of complex
        points, in the problem's length units.  raw: (n, 2), the two results
        per contour; missed: per contour the samples no element contains
        (they add nothing).  Every contour's result has the bits it has when
        integrated alone."""
        xy = [self._contour_xy(c) for c in contours]
        n = len(xy)
        ptr = np.zeros(n + 1, np.int32)
        ptr[1:] = np.cumsum([len(x) for x, _ in xy])
        x = np.ascontiguousarray(np.concatenate([x for x, _ in xy] + [np.zeros(1)]))
        y = np.ascontiguousarray(np.concatenate([y for _, y in xy] + [np.zeros(1)]))
        o = np.zeros((max(1, n), 2))
        missed = np.zeros(max(1, n), np.int32)
        _check(_lib.xfk_pot_line_integrals(self._h, n, ptr.ctypes.data_as(iptr), x.ctypes.data_as(dptr),
                                           y.ctypes.data_as(dptr), int(kind), int(bool(smooth)), int(points),
                                           o.ctypes.data_as(dptr), missed.ctypes.data_as(iptr)))
        return {"raw": o[:n], "missed": missed[:n]}

    def line_integral(self, contour, kind: int, smooth: bool = True, points: int = 400) -> complex:
        """One contour's lineIntegral of type `kind`: the two results as a
        complex number (xfk_pot_line_integral)."""
        x, y = self._contour_xy(contour)
        o = np.zeros(2)
        _check(_lib.xfk_pot_line_integral(self._h, len(x), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(kind),
                                          int(bool(smooth)), int(points), o.ctypes.data_as(dptr), None))
        return complex(o[0], o[1])

    def contour_samples(self, contour, kind: int, points: int = 400) -> dict:
        """Diagnostic: the samples of one contour as the kernel makes them, xy
        (n, 2) and the element each took, -1 for none (xfk_pot_contour_samples)."""
        x, y = self._contour_xy(contour)
        ns = max(0, len(x) - 1) * (int(points) if points > 0 else 400)
        xy = np.zeros((max(1, ns), 2))
        el = np.zeros(max(1, ns), np.int32)
        _check(_lib.xfk_pot_contour_samples(self._h, len(x), x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), int(kind),
                                            int(points), xy.ctypes.data_as(dptr), el.ctypes.data_as(iptr)))
        return {"xy": xy[:ns], "elem": el[:ns]}

    def time_contours(self, contours, kind: int, smooth: bool = True, points: int = 400, repeats: int = 5) -> float:
        """Diagnostic: HIP-event ms (median) of the contour kernel and its sums
        over the batch (xfk_pot_contour_time)."""
        xy = [self._contour_xy(c) for c in contours]
        ptr = np.zeros(len(xy) + 1, np.int32)
        ptr[1:] = np.cumsum([len(x) for x, _ in xy])
        x = np.ascontiguousarray(np.concatenate([x for x, _ in xy]))
        y = np.ascontiguousarray(np.concatenate([y for _, y in xy]))
        ms = C.c_double()
        _check(_lib.xfk_pot_contour_time(self._h, len(xy), ptr.ctypes.data_as(iptr), x.ctypes.data_as(dptr),
                                         y.ctypes.data_as(dptr), int(kind), int(bool(smooth)), int(points),
                                         int(repeats), C.byref(ms)))
        return ms.value


class ElectrostaticProblem(_PotentialPostProc):
    """One device-resident electrostatic problem (ESolver::AnalyzeProblem).

    Arrays follow the reference's in-memory state after ESolver::LoadMesh and
    LoadProblemFile: coordinates in mm, 0-based indices, -1 for "none".
    blocks: ex, ey, qv; labels: block, is_external; lines: format (0 fixed V,
    1 mixed, 2 surface charge), V, qs, c0, c1; points: V, qp; conductors:
    type (1 prescribed V, 0 prescribed total charge q), V, q.  marker /
    conductor: per node, the point property / conductor index.  depth and
    ext_* in the problem's length units."""

    _POINT_NAMES = (("V", 0), ("D", [1, 2]), ("E", [3, 4]), ("e", [5, 6]), ("nrg", 7))

    def __init__(self, *, x, y, p, lbl, blocks: Sequence[dict], labels: Sequence[dict],
                 lines: Sequence[dict] = (), points: Sequence[dict] = (), conductors: Sequence[dict] = (),
                 marker=None, conductor=None, e=None, pbc=None, precision=1e-8, length_units=0,
                 problem_type: int = 0, depth: float = 1.0, ext_zo: float = 0.0, ext_ro: float = 0.0,
                 ext_ri: float = 0.0, device=0, precond: str = "amg"):
        L = load_library()
        keep = _Keep()
        bl = (EsBlockDesc * max(1, len(blocks)))()
        for k, b in enumerate(blocks):
            bl[k].ex, bl[k].ey, bl[k].qv = b.get("ex", 1.0), b.get("ey", 1.0), b.get("qv", 0.0)
        lb = (EsLabelDesc * max(1, len(labels)))()
        for k, l in enumerate(labels):
            lb[k].block, lb[k].is_external = l["block"], int(l.get("is_external", 0))
        ln = (EsLineDesc * max(1, len(lines)))()
        for k, l in enumerate(lines):
            ln[k].format, ln[k].V, ln[k].qs = l.get("format", 0), l.get("V", 0.0), l.get("qs", 0.0)
            ln[k].c0, ln[k].c1 = l.get("c0", 0.0), l.get("c1", 0.0)
        pt = (EsPointDesc * max(1, len(points)))()
        for k, q in enumerate(points):
            pt[k].V, pt[k].qp = q.get("V", 0.0), q.get("qp", 0.0)
        co = (EsConductorDesc * max(1, len(conductors)))()
        for k, q in enumerate(conductors):
            co[k].type, co[k].V, co[k].q = q.get("type", 1), q.get("V", 0.0), q.get("q", 0.0)
        D = EsProblemDesc()
        x = np.asarray(x, dtype=np.float64)
        D.n_nodes = len(x)
        D.x, D.y = keep.d(x), keep.d(y)
        D.marker = keep.i(marker) if marker is not None else None
        D.conductor = keep.i(conductor) if conductor is not None else None
        p = np.asarray(p, dtype=np.int32).reshape(-1)
        D.n_elems = len(p) // 3
        D.p = keep.i(p)
        D.e = keep.i(np.asarray(e, dtype=np.int32).reshape(-1)) if e is not None else None
        D.lbl = keep.i(lbl)
        D.n_blocks, D.blocks = len(blocks), bl
        D.n_labels, D.labels = len(labels), lb
        D.n_lines, D.lines = len(lines), ln
        D.n_points, D.points = len(points), pt
        D.n_conductors, D.conductors = len(conductors), co
        if pbc is not None and len(pbc):
            pb = np.asarray(pbc, dtype=np.int32).reshape(-1)
            D.n_pbc, D.pbc = len(pb) // 3, keep.i(pb)
        else:
            D.n_pbc, D.pbc = 0, None
        D.precision, D.length_units, D.problem_type = precision, int(length_units), int(problem_type)
        D.depth, D.ext_zo, D.ext_ro, D.ext_ri = depth, ext_zo, ext_ro, ext_ri
        keep.extend([bl, lb, ln, pt, co])
        self._keep = keep
        self.n_nodes = self.n_rows = D.n_nodes
        self.n_elems = D.n_elems
        self.n_conductors = len(conductors)
        self.n_labels = len(labels)
        h = C.c_void_p()
        _check(L.xfk_problem_create_electrostatic(C.byref(D), device, C.byref(h)))
        self._h = h
        self.set_option(XFK_OPT_PRECOND, PRECONDS[precond])
        self.result: Optional[Result] = None

    set_option = Static2DProblem.set_option
    memory = Static2DProblem.memory
    close = Static2DProblem.close
    __del__ = Static2DProblem.__del__
    csr = Static2DProblem.csr

    def solve(self, rebuild_symbolic: bool = False) -> dict:
        r = Result()
        _check(_lib.xfk_electrostatic(self._h, XFK_REBUILD_SYMBOLIC if rebuild_symbolic else 0, C.byref(r)))
        self.result = r
        return r.as_dict()

    def solution(self) -> np.ndarray:
        """V at every node."""
        V = np.zeros(self.n_nodes)
        _check(_lib.xfk_get_solution(self._h, V.ctypes.data_as(dptr)))
        return V

    def conductors(self):
        """(V, q) per conductor: the prescribed or solved potential, the
        integrated or prescribed charge (xfk_get_conductors)."""
        n = self.n_conductors
        V = np.zeros(max(1, n))
        q = np.zeros(max(1, n))
        _check(_lib.xfk_get_conductors(self._h, V.ctypes.data_as(dptr), q.ctypes.data_as(dptr)))
        return V[:n], q[:n]

    def conductor_charge(self, i: int) -> float:
        """ChargeOnConductor(i) of the last solution (xfk_conductor_charge)."""
        q = C.c_double()
        _check(_lib.xfk_conductor_charge(self._h, int(i), C.byref(q)))
        return q.value

    # -- the weighted stress tensor force and torque (block integrals 5 and 6) --

    def _mask_args(self, selected_labels, selected_nodes, max_area):
        sel, _ = self._mask(selected_labels)
        nodes = None
        if selected_nodes is not None:
            nodes = np.zeros(self.n_nodes, np.uint8)
            s = np.asarray(selected_nodes)
            if s.dtype == np.bool_:
                if s.shape != (self.n_nodes,):
                    raise ValueError("expected one flag per node (%d), got shape %s" % (self.n_nodes, s.shape))
                nodes[:] = s
            else:
                nodes[s.astype(np.int64)] = 1
        area = None
        if max_area is not None:
            area = np.ascontiguousarray(max_area, dtype=np.float64)
            if area.shape != (self.n_labels,):
                raise ValueError("expected one MaxArea per label (%d), got shape %s" % (self.n_labels, area.shape))
        return sel, nodes, area

    def mask_info(self) -> dict:
        """Whether the problem holds a mask, and the last make_mask's PCG
        iterations and times in ms (xfk_pot_mask_info)."""
        o = np.zeros(9)
        _check(_lib.xfk_pot_mask_info(self._h, o.ctypes.data_as(dptr)))
        return dict(ready=bool(o[0]), cg_iters=int(o[1]),
                    times=dict(create=o[2], fixed_values=o[3], symbolic=o[4], assemble=o[5], amg_setup=o[6],
                               solve=o[7], total=o[8]))

    def make_mask(self, selected_labels, selected_nodes=None, max_area=None) -> dict:
        """PostProcessor::makeMask for the selected labels (indices or a boolean
        mask per label) and nodes (likewise); max_area: the labels' MaxArea
        (None: the element areas weight the Laplacian).  Returns W (the solved
        nodal values), msk (W > 0.5 as 0 / 1), cg_iters and times (ms)."""
        ubp = C.POINTER(C.c_ubyte)
        sel, nodes, area = self._mask_args(selected_labels, selected_nodes, max_area)
        self._mask_key = None
        _check(_lib.xfk_pot_make_mask(self._h, None if sel is None else sel.ctypes.data_as(ubp),
                                      None if nodes is None else nodes.ctypes.data_as(ubp),
                                      None if area is None else area.ctypes.data_as(dptr)))
        self._mask_key = tuple(None if a is None else a.tobytes() for a in (sel, nodes, area))
        W = np.zeros(self.n_nodes)
        msk = np.zeros(self.n_nodes)
        _check(_lib.xfk_pot_get_mask(self._h, W.ctypes.data_as(dptr), msk.ctypes.data_as(dptr)))
        info = self.mask_info()
        return dict(W=W, msk=msk, cg_iters=info["cg_iters"], times=info["times"])

    def mask_csr(self):
        """Diagnostic: the assembled system of the last mask solve, as csr()."""
        h = C.c_void_p()
        _check(_lib.xfk_pot_mask_problem(self._h, C.byref(h)))
        nnz = _lib.xfk_get_nnz(h)
        rp = np.zeros(self.n_nodes + 1, np.int32)
        col = np.zeros(nnz, np.int32)
        val = np.zeros(nnz)
        b = np.zeros(self.n_nodes)
        _check(_lib.xfk_get_csr(h, rp.ctypes.data_as(iptr), col.ctypes.data_as(iptr), val.ctypes.data_as(dptr),
                                b.ctypes.data_as(dptr)))
        return rp, col, val, b

    def weighted_stress(self, selected_labels, selected_nodes=None, max_area=None) -> dict:
        """The weighted stress tensor force (N) and torque about the origin
        (N m) on the selection: block integrals 5 and 6, the mask made first
        unless the problem holds the one of these very arguments."""
        key = tuple(None if a is None else a.tobytes()
                    for a in self._mask_args(selected_labels, selected_nodes, max_area))
        if getattr(self, "_mask_key", None) != key or not self.mask_info()["ready"]:
            self.make_mask(selected_labels, selected_nodes, max_area)
        f = self.block_integral(selected_labels, 5)
        t = self.block_integral(selected_labels, 6)
        return dict(force=np.array([f.real, f.imag]), torque=t.real)

    def time_stress(self, repeats: int = 5) -> float:
        """Diagnostic: HIP-event ms (median) of the integral launch of types 5 and 6."""
        ms = C.c_double()
        _check(_lib.xfk_pot_stress_time(self._h, int(repeats), C.byref(ms)))
        return ms.value


class HeatFlowProblem(_PotentialPostProc):
    """One device-resident heat-flow problem (HSolver::AnalyzeProblem).

    Arrays follow the reference's in-memory state after HSolver::LoadMesh and
    LoadProblemFile: coordinates in m, 0-based indices, -1 for "none".
    blocks: kx, ky, kt, qv and an optional K(T) table T, K; labels: block,
    is_external; lines: format (0 fixed Tset, 1 flux qs, 2 convection h Tinf,
    3 radiation beta Tinf), points: T, qp; conductors: type (1 prescribed T,
    0 prescribed total heat flow q), T, q.  marker / conductor: per node, the
    point property / conductor index.  depth and ext_* in the problem's length
    units.  dt, t_prev: the time step and the previous solution (0: steady)."""

    _FIELD_NAMES = ("F", "G")
    _INTEGRAL_NAMES = ("T", "area", "volume", "F", "G")
    _POINT_NAMES = (("T", 0), ("F", [1, 2]), ("K", [3, 4]), ("G", [5, 6]))

    def __init__(self, *, x, y, p, lbl, blocks: Sequence[dict], labels: Sequence[dict],
                 lines: Sequence[dict] = (), points: Sequence[dict] = (), conductors: Sequence[dict] = (),
                 marker=None, conductor=None, e=None, pbc=None, precision=1e-8, length_units=0,
                 problem_type: int = 0, depth: float = 1.0, ext_zo: float = 0.0, ext_ro: float = 0.0,
                 ext_ri: float = 0.0, dt: float = 0.0, t_prev=None, device=0, precond: str = "amg"):
        L = load_library()
        keep = _Keep()
        bl = (HfBlockDesc * max(1, len(blocks)))()
        for k, b in enumerate(blocks):
            bl[k].kx, bl[k].ky = b.get("kx", 1.0), b.get("ky", 1.0)
            bl[k].kt, bl[k].qv = b.get("kt", 0.0), b.get("qv", 0.0)
            bl[k].npts = int(b["npts"]) if "npts" in b else len(b.get("T", ()))
            bl[k].T = keep.d(b["T"]) if b.get("T") is not None and len(b["T"]) else None
            bl[k].K = keep.d(b["K"]) if b.get("K") is not None and len(b["K"]) else None
        lb = (HfLabelDesc * max(1, len(labels)))()
        for k, l in enumerate(labels):
            lb[k].block, lb[k].is_external = l["block"], int(l.get("is_external", 0))
        ln = (HfLineDesc * max(1, len(lines)))()
        for k, l in enumerate(lines):
            ln[k].format, ln[k].Tset, ln[k].qs = l.get("format", 0), l.get("Tset", 0.0), l.get("qs", 0.0)
            ln[k].beta, ln[k].h, ln[k].Tinf = l.get("beta", 0.0), l.get("h", 0.0), l.get("Tinf", 0.0)
        pt = (HfPointDesc * max(1, len(points)))()
        for k, q in enumerate(points):
            pt[k].T, pt[k].qp = q.get("T", 0.0), q.get("qp", 0.0)
        co = (HfConductorDesc * max(1, len(conductors)))()
        for k, q in enumerate(conductors):
            co[k].type, co[k].T, co[k].q = q.get("type", 1), q.get("T", 0.0), q.get("q", 0.0)
        D = HfProblemDesc()
        x = np.asarray(x, dtype=np.float64)
        D.n_nodes = len(x)
        D.x, D.y = keep.d(x), keep.d(y)
        D.marker = keep.i(marker) if marker is not None else None
        D.conductor = keep.i(conductor) if conductor is not None else None
        p = np.asarray(p, dtype=np.int32).reshape(-1)
        D.n_elems = len(p) // 3
        D.p = keep.i(p)
        D.e = keep.i(np.asarray(e, dtype=np.int32).reshape(-1)) if e is not None else None
        D.lbl = keep.i(lbl)
        D.n_blocks, D.blocks = len(blocks), bl
        D.n_labels, D.labels = len(labels), lb
        D.n_lines, D.lines = len(lines), ln
        D.n_points, D.points = len(points), pt
        D.n_conductors, D.conductors = len(conductors), co
        if pbc is not None and len(pbc):
            pb = np.asarray(pbc, dtype=np.int32).reshape(-1)
            D.n_pbc, D.pbc = len(pb) // 3, keep.i(pb)
        else:
            D.n_pbc, D.pbc = 0, None
        D.precision, D.length_units, D.problem_type = precision, int(length_units), int(problem_type)
        D.depth, D.ext_zo, D.ext_ro, D.ext_ri = depth, ext_zo, ext_ro, ext_ri
        D.dt = dt
        D.t_prev = keep.d(self._nodal(t_prev, D.n_nodes)) if t_prev is not None else None
        keep.extend([bl, lb, ln, pt, co])
        self._keep = keep
        self.n_nodes = self.n_rows = D.n_nodes
        self.n_elems = D.n_elems
        self.n_conductors = len(conductors)
        self.n_labels = len(labels)
        h = C.c_void_p()
        _check(L.xfk_problem_create_heatflow(C.byref(D), device, C.byref(h)))
        self._h = h
        self.set_option(XFK_OPT_PRECOND, PRECONDS[precond])
        self.result: Optional[Result] = None

    set_option = Static2DProblem.set_option
    memory = Static2DProblem.memory
    close = Static2DProblem.close
    __del__ = Static2DProblem.__del__
    csr = Static2DProblem.csr

    @staticmethod
    def _nodal(v, n) -> np.ndarray:
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (n,):
            raise ValueError("expected one value per node (%d), got shape %s" % (n, v.shape))
        return v

    def solve(self, rebuild_symbolic: bool = False) -> dict:
        """The outer loop (xfk_heatflow); newton_iters of the result is the pass count."""
        r = Result()
        _check(_lib.xfk_heatflow(self._h, XFK_REBUILD_SYMBOLIC if rebuild_symbolic else 0, C.byref(r)))
        self.result = r
        return r.as_dict()

    def assemble(self, T=None):
        """One pass's system from the nodal temperatures T (None: zeros),
        without solving; csr() then shows it (xfk_heatflow_assemble)."""
        t = self._nodal(T, self.n_nodes) if T is not None else None
        _check(_lib.xfk_heatflow_assemble(self._h, t.ctypes.data_as(dptr) if t is not None else None))

    def solution(self) -> np.ndarray:
        """T at every node."""
        V = np.zeros(self.n_nodes)
        _check(_lib.xfk_get_solution(self._h, V.ctypes.data_as(dptr)))
        return V

    def set_step(self, dt: float, t_prev=None):
        """The time step and the previous solution (xfk_heatflow_set_step)."""
        t = self._nodal(t_prev, self.n_nodes) if t_prev is not None else None
        _check(_lib.xfk_heatflow_set_step(self._h, float(dt), t.ctypes.data_as(dptr) if t is not None else None))

    def advance(self, dt: float):
        """The last solution becomes the previous one, on the device (xfk_heatflow_advance)."""
        _check(_lib.xfk_heatflow_advance(self._h, float(dt)))

    def conductors(self):
        """(T, q) per conductor: the prescribed or solved temperature, the
        integrated or prescribed heat flow (xfk_hf_get_conductors)."""
        n = self.n_conductors
        T = np.zeros(max(1, n))
        q = np.zeros(max(1, n))
        _check(_lib.xfk_hf_get_conductors(self._h, T.ctypes.data_as(dptr), q.ctypes.data_as(dptr)))
        return T[:n], q[:n]

    def conductor_flow(self, i: int) -> float:
        """ChargeOnConductor(i) of the last solution (xfk_hf_conductor_flow)."""
        q = C.c_double()
        _check(_lib.xfk_hf_conductor_flow(self._h, int(i), C.byref(q)))
        return q.value


class Phase(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("calls", C.c_int), ("ms_total", C.c_double), ("bytes_per_call", C.c_double)]


XFK_PROFILE_SETUP = 1


class BlockAcDesc(C.Structure):
    _fields_ = [("J_im", C.c_double), ("Theta_hx", C.c_double), ("Theta_hy", C.c_double), ("Lam_d", C.c_double),
                ("H_im", dptr), ("slope_im", dptr)]


class LineAcDesc(C.Structure):
    _fields_ = [("c0_im", C.c_double), ("c1_im", C.c_double), ("Mu", C.c_double), ("Sig", C.c_double)]


class CircuitAcDesc(C.Structure):
    _fields_ = [("amps_im", C.c_double), ("dvolts_im", C.c_double)]


class HarmonicDesc(C.Structure):
    _fields_ = [("frequency", C.c_double), ("blocks", C.POINTER(BlockAcDesc)), ("lines", C.POINTER(LineAcDesc)),
                ("circs", C.POINTER(CircuitAcDesc)), ("ac_solver", C.c_int),
                ("label_prox_mu", C.POINTER(C.c_double)), ("prev_type", C.c_int)]


class Harmonic2DProblem(_MagPostProc):
    """One device-resident time-harmonic planar problem (FSolver::Harmonic2D).
    Same keyword arguments as Static2DProblem plus ``frequency`` (Hz) and the
    AC fields: blocks J_im, Theta_hx, Theta_hy, Lam_d; lines c0_im, c1_im, Mu,
    Sig (BdryFormat 1); circuits amps_im, dvolts_im.  The post-processing
    methods it shares with Static2DProblem are refused: they are built for
    magnetostatic problems only.  Its own are set_solution_complex,
    element_b_complex, block_integrals_complex, block_integral_complex and
    time_postproc_complex (the xfk_mag_ac_ entry points), with set_depth."""

    def __init__(self, *, x, y, p, lbl, blocks: Sequence[dict], labels: Sequence[dict], frequency: float,
                 lines: Sequence[dict] = (), points: Sequence[dict] = (), circuits: Sequence[dict] = (),
                 marker=None, e=None, pbc=None, precision=1e-8, length_units=0, coords=0, relax=1.0, device=0,
                 problem_type: int = 0, ext_zo: float = 0.0, ext_ro: float = 0.0, ext_ri: float = 0.0,
                 precond: str = "amg", ages: Sequence[dict] = (), ac_solver: int = 0,
                 comm: Optional["Comm"] = None, prev_type: int = 0):
        """prev_type: [PrevType] of the file the problem came from; the solve
        does not read it, the harmonic post-processing refuses != 0.
        precond: "amg" (V-cycle of the real SPD surrogate Re A +- Im A, the
        sign making Im A positive semi-definite, applied to the real and
        imaginary parts; default) or "jacobi" (complex Jacobi).  ac_solver:
        [ACSolver], 0 successive approximation, 1 Newton (KludgeSolve).
        comm: shard the rows over this communicator, as Static2DProblem does
        (xfk_problem_create_harmonic_dist); solution() gathers the whole field."""
        L = load_library()
        D, keep = _make_desc(x, y, p, lbl, blocks, labels, lines, points, circuits, marker, e, pbc, precision,
                             length_units, coords, relax, problem_type, (ext_zo, ext_ro, ext_ri), ages)
        ba = (BlockAcDesc * max(1, len(blocks)))()
        for k, b in enumerate(blocks):
            ba[k].J_im, ba[k].Lam_d = b.get("J_im", 0.0), b.get("Lam_d", 0.0)
            ba[k].Theta_hx, ba[k].Theta_hy = b.get("Theta_hx", 0.0), b.get("Theta_hy", 0.0)
            if len(b.get("B", ())):   # nonlinear: the complex curve of bh_get_slopes_ac
                ba[k].H_im = keep.d(np.imag(np.asarray(b["H"])))
                ba[k].slope_im = keep.d(np.imag(np.asarray(b["slope"])))
        la = (LineAcDesc * max(1, len(lines)))()
        for k, l in enumerate(lines):
            la[k].c0_im, la[k].c1_im, la[k].Mu, la[k].Sig = (l.get("c0_im", 0.0), l.get("c1_im", 0.0),
                                                             l.get("Mu", 0.0), l.get("Sig", 0.0))
        ca = (CircuitAcDesc * max(1, len(circuits)))()
        for k, q in enumerate(circuits):
            ca[k].amps_im, ca[k].dvolts_im = q.get("amps_im", 0.0), q.get("dvolts_im", 0.0)
        # labels' "prox_mu": ProximityMu after GetFillFactor (wound LamType > 2 regions)
        prox = np.zeros(2 * max(1, len(labels)))
        for k, l in enumerate(labels):
            z = complex(l.get("prox_mu", 1.0))
            prox[2 * k], prox[2 * k + 1] = z.real, z.imag
        H = HarmonicDesc(frequency, ba, la, ca, int(ac_solver), keep.d(prox), int(prev_type))
        keep.extend([ba, la, ca])
        self._keep = keep
        self.n_nodes = D.n_nodes
        self.n_elems = D.n_elems
        self.n_circs = len(circuits)
        self.n_labels = len(labels)
        h = C.c_void_p()
        self.comm = comm
        if comm is None:
            _check(L.xfk_problem_create_harmonic(C.byref(D), C.byref(H), device, C.byref(h)))
        else:
            _check(L.xfk_problem_create_harmonic_dist(C.byref(D), C.byref(H), device, comm._h, C.byref(h)))
        self._h = h
        _check(L.xfk_set_option(self._h, XFK_OPT_PRECOND, float(PRECONDS[precond])))
        self.n_rows = self.dist_info()["n_own"] if comm is not None else self.n_nodes
        self.result: Optional[Result] = None

    def solve(self, rebuild_symbolic: bool = False) -> dict:
        r = Result()
        _check(_lib.xfk_harmonic2d(self._h, XFK_REBUILD_SYMBOLIC if rebuild_symbolic else 0, C.byref(r)))
        self.result = r
        return r.as_dict()

    def memory(self) -> dict:
        """Device memory of this problem (xfk_problem_memory): arena chunk
        bytes and count, bytes carved and live, bytes kept for reuse."""
        out = (C.c_longlong * 4)()
        _check(_lib.xfk_problem_memory(self._h, out))
        return dict(chunk_bytes=int(out[0]), chunks=int(out[1]), live_bytes=int(out[2]), reuse_bytes=int(out[3]))

    def dist_info(self) -> dict:
        info = DistInfo()
        _check(_lib.xfk_dist_get_info(self._h, C.byref(info)))
        return info.as_dict()

    def solution(self) -> np.ndarray:
        A = np.zeros(2 * self.n_nodes)
        _check(_lib.xfk_get_solution_complex(self._h, A.ctypes.data_as(dptr)))
        return A[0::2] + 1j * A[1::2]

    def circuits(self):
        n = self.n_circs
        cc = np.zeros(max(1, n), np.int32)
        J = np.zeros(2 * max(1, n))
        dV = np.zeros(2 * max(1, n))
        _check(_lib.xfk_get_circuits_complex(self._h, cc.ctypes.data_as(iptr), J.ctypes.data_as(dptr),
                                             dV.ctypes.data_as(dptr)))
        return cc[:n], (J[0::2] + 1j * J[1::2])[:n], (dV[0::2] + 1j * dV[1::2])[:n]

    def csr(self):
        nnz = _lib.xfk_get_nnz(self._h)
        rp = np.zeros(self.n_rows + 1, np.int32)
        col = np.zeros(nnz, np.int32)
        val = np.zeros(2 * nnz)
        b = np.zeros(2 * self.n_rows)
        _check(_lib.xfk_get_csr_complex(self._h, rp.ctypes.data_as(iptr), col.ctypes.data_as(iptr),
                                        val.ctypes.data_as(dptr), b.ctypes.data_as(dptr)))
        return rp, col, val[0::2] + 1j * val[1::2], b[0::2] + 1j * b[1::2]

    def close(self):
        if getattr(self, "_h", None):
            load_library().xfk_problem_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pcg_solve_csr(rowptr, col, val, b, V0=None, flag=0, precision=1e-8, device=0, precond="jacobi"):
    """Stand-alone device PCG on a full symmetric CSR (CBigLinProb::PCGSolve semantics)."""
    L = load_library()
    n = len(rowptr) - 1
    rp = np.ascontiguousarray(rowptr, np.int32)
    cl = np.ascontiguousarray(col, np.int32)
    vl = np.ascontiguousarray(val, np.float64)
    bb = np.ascontiguousarray(b, np.float64)
    V = np.zeros(n) if V0 is None else np.array(V0, dtype=np.float64)
    it = C.c_longlong()
    er = C.c_double()
    _check(L.xfk_pcg_solve_csr_pc(n, rp.ctypes.data_as(iptr), cl.ctypes.data_as(iptr), vl.ctypes.data_as(dptr),
                                  bb.ctypes.data_as(dptr), V.ctypes.data_as(dptr), flag, precision, device,
                                  PRECONDS[precond], C.byref(it), C.byref(er)))
    return V, it.value, er.value


class AmgProbe:
    """Diagnostics of one AMG hierarchy built from a host CSR (xfk_amg_probe_*):
    the operators of every level as the cycle reads them, the setup's traced
    scratch, the cycle applied to given vectors and a values-only refresh.
    For tests; not an interface to build on."""

    A, P, R, PF, RF = 0, 1, 2, 3, 4
    PLAIN_COLS, F64_VALS = 16, 32
    _TRACE = {"sflag": (0, np.uint8), "sdeg": (1, np.int32), "agg": (2, np.int32), "agg_pre": (3, np.int32),
              "root": (4, np.int32), "dfinv": (5, np.float64), "wF": (6, np.float64)}

    def __init__(self, rowptr, col, val, device=0, sweeps=1, theta=0.08, omega=1.75, dense_max=2048, fold=1,
                 col16=1, f32=1, wlevel=-1, trace=False):
        L = load_library()
        self.n = len(rowptr) - 1
        rp = np.ascontiguousarray(rowptr, np.int32)
        cl = np.ascontiguousarray(col, np.int32)
        vl = np.ascontiguousarray(val, np.float64)
        self.nnz = int(rp[-1])
        o = AmgProbeOpts(sweeps, theta, omega, dense_max, int(fold), int(col16), int(f32), wlevel)
        h = C.c_void_p()
        self._h = None
        _check(L.xfk_amg_probe_create(self.n, rp.ctypes.data_as(iptr), cl.ctypes.data_as(iptr),
                                      vl.ctypes.data_as(dptr), device, C.byref(o), int(trace), C.byref(h)))
        self._h = h

    def info(self):
        I = AmgInfo()
        _check(_lib.xfk_amg_probe_info(self._h, C.byref(I)))
        lv = [{k: getattr(I.level[l], k) for k, _ in AmgLevelInfo._fields_} for l in range(I.levels)]
        return {"levels": I.levels, "dense_coarse": bool(I.dense_coarse), "cinv_f64": bool(I.cinv_f64),
                "level": lv}

    def csr(self, level, sel):
        """(shape, rowptr, col, val) of one operator of a level."""
        r, c, z = C.c_int(), C.c_int(), C.c_longlong()
        _check(_lib.xfk_amg_probe_level_size(self._h, level, sel, C.byref(r), C.byref(c), C.byref(z)))
        rp = np.zeros(r.value + 1, np.int32)
        cl = np.zeros(max(1, z.value), np.int32)
        vl = np.zeros(max(1, z.value))
        _check(_lib.xfk_amg_probe_level_csr(self._h, level, sel, rp.ctypes.data_as(iptr), cl.ctypes.data_as(iptr),
                                            vl.ctypes.data_as(dptr)))
        return (r.value, c.value), rp, cl[:z.value], vl[:z.value]

    def tiles(self, sel):
        t, w = C.c_int(), C.c_int()
        _check(_lib.xfk_amg_probe_tiles(self._h, sel, C.byref(t), C.byref(w)))
        return t.value, w.value

    def dinv(self, level):
        out = np.zeros(self.info()["level"][level]["n"])
        _check(_lib.xfk_amg_probe_vector(self._h, level, 0, out.ctypes.data_as(dptr)))
        return out

    def dense(self):
        """The n x n operator the dense coarsest level applies."""
        I = self.info()
        n = I["level"][-1]["n"]
        out = np.zeros((n, n))
        _check(_lib.xfk_amg_probe_vector(self._h, I["levels"] - 1, 1, out.ctypes.data_as(dptr)))
        return out

    def trace(self, level, name):
        what, dt = self._TRACE[name]
        lv = self.info()["level"][level]
        out = np.zeros(max(1, lv["nnz"] if name == "sflag" else lv["n"]), dt)
        _check(_lib.xfk_amg_probe_trace(self._h, level, what, out.ctypes.data_as(C.c_void_p)))
        return out[:lv["nnz"] if name == "sflag" else lv["n"]]

    def apply(self, R):
        """U[:, k] = V-cycle(R[:, k])."""
        R = np.asarray(R, np.float64)
        Rt = np.ascontiguousarray(R.reshape(self.n, -1).T)
        U = np.zeros_like(Rt)
        _check(_lib.xfk_amg_probe_apply(self._h, Rt.shape[0], Rt.ctypes.data_as(dptr), U.ctypes.data_as(dptr)))
        return np.ascontiguousarray(U.T).reshape(R.shape)

    def refresh(self, val, fold=True):
        vl = np.ascontiguousarray(val, np.float64)
        assert vl.size == self.nnz
        _check(_lib.xfk_amg_probe_refresh(self._h, vl.ctypes.data_as(dptr), int(fold)))

    def close(self):
        if getattr(self, "_h", None):
            load_library().xfk_amg_probe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CommOp(C.Structure):
    _fields_ = [("seq", C.c_longlong), ("op", C.c_int), ("stream", C.c_int), ("waited", C.c_int),
                ("peer", C.c_int), ("bytes", C.c_longlong), ("g0", C.c_longlong)]


COMM_OPS = {1: "allreduce", 2: "exchange", 3: "send", 4: "recv", 5: "allgather"}


class Comm:
    """Communicator of the sharded solve (xfk_comm): RCCL, one process per GPU,
    an in-process group of ranks driven by one host thread each, or the replay
    of one rank's recording (compute-only runs of a sharded rank)."""

    def __init__(self, handle):
        self._h = handle
        L = load_library()
        self.rank = L.xfk_comm_rank(handle)
        self.size = L.xfk_comm_size(handle)

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        _check(load_library().xfk_comm_unique_id(buf, 128))
        return buf.raw

    @classmethod
    def rccl(cls, unique_id: bytes, rank: int, size: int, device: int) -> "Comm":
        h = C.c_void_p()
        _check(load_library().xfk_comm_create_rccl(unique_id, len(unique_id), rank, size, device, C.byref(h)))
        return cls(h)

    @classmethod
    def local_group(cls, size: int) -> list:
        hs = (C.c_void_p * size)()
        _check(load_library().xfk_comm_create_local(size, hs))
        return [cls(C.c_void_p(hs[q])) for q in range(size)]

    def record(self, mode: int = 1):
        """Start an empty recording (1: the collective sequence; 2: also every
        received byte, for replay()); 0 stops it (the log stays readable)."""
        _check(load_library().xfk_comm_record(self._h, int(mode)))

    def log(self) -> list:
        """The recorded collectives: dicts seq, op (allreduce / exchange / send /
        recv / allgather), stream, waited, peer, bytes, g0 (xfk_comm_op)."""
        L = load_library()
        n = C.c_int()
        _check(L.xfk_comm_log(self._h, None, 0, C.byref(n)))
        buf = (CommOp * max(1, n.value))()
        _check(L.xfk_comm_log(self._h, C.cast(buf, C.c_void_p), n.value, C.byref(n)))
        return [dict(seq=o.seq, op=COMM_OPS.get(o.op, str(o.op)), stream=o.stream, waited=o.waited, peer=o.peer,
                     bytes=o.bytes, g0=o.g0) for o in buf[:n.value]]

    def time(self, on: bool = True):
        """Bracket every collective with HIP events (xfk_comm_time)."""
        _check(load_library().xfk_comm_time(self._h, int(bool(on))))

    def timing(self) -> dict:
        """Per op (allreduce / exchange / allgather): calls, summed and longest
        microseconds inside the collectives since the last read
        (xfk_comm_timing; waits for the events, then clears them)."""
        calls = (C.c_longlong * 3)()
        tot = (C.c_double * 3)()
        mx = (C.c_double * 3)()
        _check(load_library().xfk_comm_timing(self._h, calls, tot, mx))
        return {nm: {"calls": int(calls[k]), "us": float(tot[k]), "us_max_call": float(mx[k])}
                for k, nm in enumerate(("allreduce", "exchange", "allgather"))}

    def replay(self) -> "Comm":
        """A communicator serving this rank's mode-2 recording cyclically
        (xfk_comm_create_replay): the rank runs alone with the recorded inputs."""
        h = C.c_void_p()
        _check(load_library().xfk_comm_create_replay(self._h, C.byref(h)))
        return Comm(h)

    def close(self):
        if getattr(self, "_h", None):
            load_library().xfk_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check_comm_logs(logs) -> dict:
    """Issue-order check of one recorded program over all ranks (logs[q] =
    Comm.log() of rank q): every rank made the same sequence of collective
    calls -- op, stream index, payload bytes of all-reduces and all-gathers --
    and in every exchange each send of rank a to rank b matches a receive of b
    from a (length and first global row) in the same exchange, and the reverse.
    Raises AssertionError naming the first mismatch; returns a summary."""
    R = len(logs)
    calls = []
    for q, lg in enumerate(logs):
        cs = {}
        for o in lg:
            c = cs.setdefault(o["seq"], {"head": None, "send": [], "recv": []})
            if o["op"] in ("send", "recv"):
                c[o["op"]].append((o["peer"], o["bytes"], o["g0"]))
            else:
                c["head"] = (o["op"], o["stream"], o["bytes"] if o["op"] != "exchange" else 0)
        calls.append([cs[k] for k in sorted(cs)])
    n = len(calls[0])
    for q in range(1, R):
        assert len(calls[q]) == n, "rank %d made %d collective calls, rank 0 %d" % (q, len(calls[q]), n)
    waits = 0
    streams = set()
    for k in range(n):
        h0 = calls[0][k]["head"]
        for q in range(1, R):
            assert calls[q][k]["head"] == h0, "call %d: rank 0 %s, rank %d %s" % (k, h0, q, calls[q][k]["head"])
        streams.add(h0[1])
        if h0[0] != "exchange":
            continue
        for a in range(R):
            for (b, nb, g0) in calls[a][k]["send"]:
                assert (a, nb, g0) in calls[b][k]["recv"], \
                    "exchange %d: rank %d sends %d B (row %d) to %d, which posts no such receive" % (k, a, nb, g0, b)
            for (b, nb, g0) in calls[a][k]["recv"]:
                assert (a, nb, g0) in calls[b][k]["send"], \
                    "exchange %d: rank %d expects %d B (row %d) from %d, which sends no such range" % (k, a, nb, g0, b)
    for lg in logs:
        prev = None
        for o in lg:
            if o["op"] in ("send", "recv"):
                continue
            if prev is not None and o["stream"] != prev:
                assert o["waited"] == 1, "call %d changes stream without the ordering wait" % o["seq"]
            waits += o["waited"]
            prev = o["stream"]
    ops = {}
    for c in calls[0]:
        ops[c["head"][0]] = ops.get(c["head"][0], 0) + 1
    return {"calls": n, "ops": ops, "streams": sorted(streams), "stream_switches": waits}


def partition_plan(n_nodes: int, p, rank: int, nranks: int, coupled=None) -> dict:
    """Host-only row-block partition plan of xfk_problem_create_dist (no device);
    ``coupled``: periodic / air-gap nodes (xfk_partition_plan_coupled)."""
    L = load_library()
    p = np.ascontiguousarray(np.asarray(p, dtype=np.int32).reshape(-1))
    ne = len(p) // 3
    info = DistInfo()
    pp = p.ctypes.data_as(iptr)
    cp = np.ascontiguousarray(np.asarray([] if coupled is None else coupled, dtype=np.int32).reshape(-1))
    nc = len(cp)
    cpp = cp.ctypes.data_as(iptr) if nc else None
    _check(L.xfk_partition_plan_coupled(n_nodes, ne, pp, rank, nranks, nc, cpp, C.byref(info), None, None, None,
                                        None))
    l2g = np.zeros(info.n_own + info.n_halo, np.int32)
    elems = np.zeros(max(1, info.n_elems), np.int32)
    recv = np.zeros(4 * max(1, info.n_recv), np.int32)
    send = np.zeros(4 * max(1, info.n_send), np.int32)
    _check(L.xfk_partition_plan_coupled(n_nodes, ne, pp, rank, nranks, nc, cpp, C.byref(info),
                                        l2g.ctypes.data_as(iptr), elems.ctypes.data_as(iptr),
                                        recv.ctypes.data_as(iptr), send.ctypes.data_as(iptr)))
    d = info.as_dict()
    d["l2g"] = l2g
    d["elems"] = elems[:info.n_elems]
    d["recv"] = recv[:4 * info.n_recv].reshape(-1, 4)   # peer, local offset, length, first global row
    d["send"] = send[:4 * info.n_send].reshape(-1, 4)
    return d
