"""Python view of the file-based ESolver and HSolver (include/xfemm_psolver.h).

Mirrors the reference's solver surface (cfemm/esolver/esolver.h,
cfemm/hsolver/hsolver.h) with the same names: ``PathName``,
``LoadProblemFile()``, ``runSolver(verbose)``, ``LoadMesh()``, ``Cuthill()``.
A .fee / .feh with its mesh files goes in, a .res / .anh comes out.  The solve
runs on the GPU; there is no CPU fallback.  ``problem()`` gives the solved
problem as a kernels.ElectrostaticProblem / HeatFlowProblem around the live
handle, so post-processing needs no reload.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import fsolver, kernels

_COMMON = (
    "create", "destroy", "set_message_handlers", "set_pathname", "set_device", "set_delete_mesh_files",
    "load_problem_file", "run_solver", "load_mesh", "cuthill", "get_nodes", "get_element_edges", "get_pbcs",
    "num_pbcs", "bandwidth", "num_nodes", "num_elements", "get_solution", "get_elements", "num_conductors",
    "get_conductors", "get_stats", "get_times", "last_error", "problem", "get_header", "num_line_props",
    "num_node_props", "num_block_props", "num_block_labels", "get_point_prop", "get_line_prop", "get_block_prop",
    "get_conductor_prop", "get_block_label", "get_block_table",
)
EXPORTED = tuple("xfemm_%s_%s" % (s, f) for s in ("esolver", "hsolver") for f in _COMMON) + (
    "xfemm_hsolver_set_previous_solution", "xfemm_hsolver_previous_solution_file")

_lib = None
dptr = kernels.dptr
iptr = kernels.iptr


def load_library():
    """The solvers live in libxfemm_fsolver.so, beside FSolver."""
    global _lib
    if _lib is not None:
        return _lib
    L = fsolver.load_library()
    vp = C.c_void_p
    if not hasattr(L, "xfemm_esolver_create"):
        raise kernels.XfkError("%s has no ESolver / HSolver (rebuild: __graft_entry__.build())" % fsolver.FSOLVER_SO)
    for s in ("esolver", "hsolver"):
        f = lambda nm: getattr(L, "xfemm_%s_%s" % (s, nm))   # noqa: E731
        f("create").restype = vp
        f("problem").restype = vp
        f("last_error").restype = C.c_char_p
        for nm in _COMMON:
            if nm != "create":
                f(nm).argtypes = [vp]
        f("destroy").restype = None
        f("set_pathname").argtypes = [vp, C.c_char_p]
        f("set_device").argtypes = [vp, C.c_int]
        f("set_delete_mesh_files").argtypes = [vp, C.c_int]
        f("run_solver").argtypes = [vp, C.c_int]
        f("get_nodes").argtypes = [vp, dptr, dptr, iptr, iptr]
        f("get_element_edges").argtypes = [vp, iptr]
        f("get_pbcs").argtypes = [vp, iptr]
        f("get_solution").argtypes = [vp, dptr, dptr, dptr, iptr]
        f("get_elements").argtypes = [vp, iptr, iptr]
        f("get_conductors").argtypes = [vp, dptr, dptr]
        f("get_stats").argtypes = [vp, C.POINTER(kernels.Result)]
        f("get_times").argtypes = [vp, C.POINTER(C.c_double)]
        f("get_header").argtypes = [vp, dptr]
        for nm in ("get_point_prop", "get_line_prop", "get_block_prop", "get_conductor_prop", "get_block_label"):
            f(nm).argtypes = [vp, C.c_int, dptr]
        f("get_block_table").argtypes = [vp, C.c_int, dptr, dptr]
        f("set_message_handlers").argtypes = [vp, vp, vp]
        f("set_message_handlers").restype = None
    L.xfemm_hsolver_set_previous_solution.argtypes = [vp, dptr, C.c_int]
    L.xfemm_hsolver_previous_solution_file.argtypes = [vp]
    L.xfemm_hsolver_previous_solution_file.restype = C.c_char_p
    _lib = L
    return L


class _Borrowed:
    """Mixin: the handle belongs to the solver object, which outlives this view."""

    def close(self):
        self._h = None

    def __del__(self):
        pass


class _PSolver:
    _name = ""
    _problem_class = None

    def __init__(self, device: int = 0, delete_mesh_files: bool = True):
        load_library()
        self._h = C.c_void_p(self._f("create")())
        self._f("set_device")(self._h, device)
        self._f("set_delete_mesh_files")(self._h, int(delete_mesh_files))
        self._path = ""

    def _f(self, nm):
        return getattr(_lib, "xfemm_%s_%s" % (self._name, nm))

    def __del__(self):
        try:
            if self._h:
                self._f("destroy")(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def PathName(self) -> str:
        return self._path

    @PathName.setter
    def PathName(self, p: str):
        self._path = p
        self._f("set_pathname")(self._h, p.encode())

    def LoadProblemFile(self) -> bool:
        return bool(self._f("load_problem_file")(self._h))

    def LoadMesh(self) -> bool:
        return bool(self._f("load_mesh")(self._h))

    def Cuthill(self) -> bool:
        return bool(self._f("cuthill")(self._h))

    def runSolver(self, verbose: bool = False) -> bool:
        return bool(self._f("run_solver")(self._h, int(verbose)))

    def last_error(self) -> str:
        return self._f("last_error")(self._h).decode()

    @property
    def NumNodes(self) -> int:
        return self._f("num_nodes")(self._h)

    @property
    def NumEls(self) -> int:
        return self._f("num_elements")(self._h)

    @property
    def BandWidth(self) -> int:
        return self._f("bandwidth")(self._h)

    def header(self) -> dict:
        """What LoadProblemFile read from the header tokens."""
        o = np.zeros(8)
        self._f("get_header")(self._h, o.ctypes.data_as(dptr))
        return dict(precision=o[0], depth=o[1], length_units=int(o[2]), problem_type=int(o[3]), ext_zo=o[4],
                    ext_ro=o[5], ext_ri=o[6], dt=o[7])

    def _props(self, count, getter, width):
        out = []
        for k in range(self._f(count)(self._h)):
            o = np.zeros(width)
            self._f(getter)(self._h, k, o.ctypes.data_as(dptr))
            out.append(o)
        return out

    def labels(self) -> list:
        return [dict(block=int(o[0]), is_external=int(o[1]), is_default=int(o[2]))
                for o in self._props("num_block_labels", "get_block_label", 3)]

    def nodes(self):
        """x, y (the solver's unit), point property and conductor of every node."""
        n = self.NumNodes
        x, y = np.zeros(n), np.zeros(n)
        m, c = np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._f("get_nodes")(self._h, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), m.ctypes.data_as(iptr),
                             c.ctypes.data_as(iptr))
        return x, y, m, c

    def elements(self):
        ne = self.NumEls
        p = np.zeros((ne, 3), np.int32)
        lbl = np.zeros(ne, np.int32)
        e = np.zeros((ne, 3), np.int32)
        self._f("get_elements")(self._h, p.ctypes.data_as(iptr), lbl.ctypes.data_as(iptr))
        self._f("get_element_edges")(self._h, e.ctypes.data_as(iptr))
        return p, lbl, e

    def pbcs(self):
        n = self._f("num_pbcs")(self._h)
        a = np.zeros((max(n, 1), 3), np.int32)
        self._f("get_pbcs")(self._h, a.ctypes.data_as(iptr))
        return a[:n]

    def solution(self):
        """x, y (the problem's length units), the potential and the Q mark of every node."""
        n = self.NumNodes
        x, y, V = np.zeros(n), np.zeros(n), np.zeros(n)
        Q = np.zeros(n, np.int32)
        if not self._f("get_solution")(self._h, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr),
                                       V.ctypes.data_as(dptr), Q.ctypes.data_as(iptr)):
            raise RuntimeError("no solution")
        return x, y, V, Q

    def conductors(self):
        """(V, q) of the conductor lines of the output file."""
        n = self._f("num_conductors")(self._h)
        V, q = np.zeros(max(1, n)), np.zeros(max(1, n))
        if not self._f("get_conductors")(self._h, V.ctypes.data_as(dptr), q.ctypes.data_as(dptr)):
            raise RuntimeError("no solution")
        return V[:n], q[:n]

    def times(self) -> dict:
        """Wall milliseconds of the last runSolver: load_mesh, cuthill, create
        (descriptor + upload), solve (device + read-back), write."""
        ms = (C.c_double * 5)()
        self._f("get_times")(self._h, ms)
        return dict(zip(("ms_load_mesh", "ms_cuthill", "ms_create", "ms_solve", "ms_write"), list(ms)))

    def stats(self) -> dict:
        r = kernels.Result()
        self._f("get_stats")(self._h, C.byref(r))
        return r.as_dict()

    def problem(self):
        """The solved problem on the device as its kernels class, around the
        live handle (owned by this solver: valid until its next run)."""
        h = self._f("problem")(self._h)
        if not h:
            raise RuntimeError("no solved problem (runSolver first)")
        cls = type("FileSolved" + self._problem_class.__name__, (_Borrowed, self._problem_class), {})
        P = cls.__new__(cls)
        P._h = C.c_void_p(h)
        P._owner = self
        P.n_nodes = P.n_rows = self.NumNodes
        P.n_elems = self.NumEls
        P.n_conductors = self._f("num_conductors")(self._h)
        P.n_labels = self._f("num_block_labels")(self._h)
        P.result = None
        return P


class ESolver(_PSolver):
    """The reference ESolver workflow over the MI355X hot path: .fee in, .res out."""
    _name = "esolver"
    _problem_class = kernels.ElectrostaticProblem

    def kw(self) -> dict:
        """The keyword dictionary of kernels.ElectrostaticProblem for the
        loaded (and, after Cuthill, renumbered) problem."""
        x, y, m, c = self.nodes()
        p, lbl, e = self.elements()
        h = self.header()
        nl, npt = len(self._props("num_line_props", "get_line_prop", 8)), self._f("num_node_props")(self._h)
        nc = self._f("num_conductors")(self._h)
        return dict(
            x=x, y=y, p=p, lbl=lbl, e=np.where((e >= 0) & (e < nl), e, -1).astype(np.int32),
            marker=np.where(m < npt, m, -1).astype(np.int32), conductor=np.where(c < nc, c, -1).astype(np.int32),
            pbc=self.pbcs(),
            blocks=[dict(ex=o[0], ey=o[1], qv=o[3]) for o in self._props("num_block_props", "get_block_prop", 5)],
            labels=[dict(block=max(0, l["block"]), is_external=l["is_external"]) for l in self.labels()],
            lines=[dict(format=int(o[0]), V=o[1], qs=o[2], c0=o[3], c1=o[4])
                   for o in self._props("num_line_props", "get_line_prop", 8)],
            points=[dict(V=o[0], qp=o[1]) for o in self._props("num_node_props", "get_point_prop", 2)],
            conductors=[dict(type=int(o[0]), V=o[1], q=o[2])
                        for o in self._props("num_conductors", "get_conductor_prop", 3)],
            precision=h["precision"], length_units=h["length_units"], problem_type=h["problem_type"],
            depth=h["depth"], ext_zo=h["ext_zo"], ext_ro=h["ext_ro"], ext_ri=h["ext_ri"])


class HSolver(_PSolver):
    """The reference HSolver workflow over the MI355X hot path: .feh in, .anh out."""
    _name = "hsolver"
    _problem_class = kernels.HeatFlowProblem

    @property
    def previousSolutionFile(self) -> str:
        return _lib.xfemm_hsolver_previous_solution_file(self._h).decode()

    def set_previous_solution(self, T) -> bool:
        """The previous time step's temperatures, one per node in the order of
        the .node file (None: none).  A [PrevSoln] file is never read."""
        if T is None:
            return bool(_lib.xfemm_hsolver_set_previous_solution(self._h, None, 0))
        t = np.ascontiguousarray(T, dtype=np.float64)
        return bool(_lib.xfemm_hsolver_set_previous_solution(self._h, t.ctypes.data_as(dptr), len(t)))

    def kw(self) -> dict:
        """The keyword dictionary of kernels.HeatFlowProblem for the loaded
        (and, after Cuthill, renumbered) problem; without dt / t_prev."""
        x, y, m, c = self.nodes()
        p, lbl, e = self.elements()
        h = self.header()
        nl, npt = self._f("num_line_props")(self._h), self._f("num_node_props")(self._h)
        nc = self._f("num_conductors")(self._h)
        blocks = []
        for k, o in enumerate(self._props("num_block_props", "get_block_prop", 5)):
            b = dict(kx=o[0], ky=o[1], kt=o[2], qv=o[3])
            n = int(o[4])
            if n:
                T, K = np.zeros(n), np.zeros(n)
                self._f("get_block_table")(self._h, k, T.ctypes.data_as(dptr), K.ctypes.data_as(dptr))
                b.update(T=T, K=K)
            blocks.append(b)
        return dict(
            x=x, y=y, p=p, lbl=lbl, e=np.where((e >= 0) & (e < nl), e, -1).astype(np.int32),
            marker=np.where(m < npt, m, -1).astype(np.int32), conductor=np.where(c < nc, c, -1).astype(np.int32),
            pbc=self.pbcs(), blocks=blocks,
            labels=[dict(block=max(0, l["block"]), is_external=l["is_external"]) for l in self.labels()],
            lines=[dict(format=int(o[0]), Tset=o[1], qs=o[2], beta=o[5], h=o[6], Tinf=o[7])
                   for o in self._props("num_line_props", "get_line_prop", 8)],
            points=[dict(T=o[0], qp=o[1]) for o in self._props("num_node_props", "get_point_prop", 2)],
            conductors=[dict(type=int(o[0]), T=o[1], q=o[2])
                        for o in self._props("num_conductors", "get_conductor_prop", 3)],
            precision=h["precision"], length_units=h["length_units"], problem_type=h["problem_type"],
            depth=h["depth"], ext_zo=h["ext_zo"], ext_ro=h["ext_ro"], ext_ri=h["ext_ri"])
