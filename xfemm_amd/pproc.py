"""Python view of the file-based post-processors EPProc and HPProc
(include/xfemm_pproc.h): a .res / .anh goes in, the reference's epproc /
hpproc quantities come out.  ``read()`` is the host-only step; ``open()`` also
puts the problem on the GPU with the file's solution and Q marks loaded (there
is no CPU fallback).  ``problem()`` gives the opened problem as a
kernels.ElectrostaticProblem / HeatFlowProblem around the live handle, for the
xfk_pot_* calls; it cannot be solved: the file holds no boundary conditions.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import fsolver, kernels
from .psolver import _Borrowed

_FUNCS = (
    "create", "destroy", "set_device", "set_message_handlers", "read", "num_nodes", "num_elements", "num_conductors",
    "get_nodes", "get_elements", "get_conductors", "get_header", "num_line_props", "num_node_props",
    "num_block_props", "num_block_labels", "get_block_label", "get_block_prop", "geometry_counts",
    "get_geometry_points", "get_geometry_segments", "get_geometry_arcs", "open_document", "clear_selection",
    "select_block_label", "toggle_label", "toggle_group", "get_selection", "set_smoothing", "block_integral",
    "get_point_values", "get_point_values_batch", "add_contour_point", "add_contour_point_from_node", "bend_contour",
    "clear_contour", "num_contour_points", "get_contour", "line_integral", "plot_bounds",
    "has_multiply_defined_labels", "problem", "last_error",
)
EXPORTED = tuple("xfemm_%s_%s" % (s, f) for s in ("epproc", "hpproc") for f in _FUNCS)

_lib = None
dptr = kernels.dptr
iptr = kernels.iptr
ubptr = C.POINTER(C.c_ubyte)


def load_library():
    """The post-processors live in libxfemm_fsolver.so, beside the solvers."""
    global _lib
    if _lib is not None:
        return _lib
    L = fsolver.load_library()
    vp, d, i = C.c_void_p, C.c_double, C.c_int
    if not hasattr(L, "xfemm_epproc_create"):
        raise kernels.XfkError("%s has no EPProc / HPProc (rebuild: __graft_entry__.build())" % fsolver.FSOLVER_SO)
    for s in ("epproc", "hpproc"):
        f = lambda nm: getattr(L, "xfemm_%s_%s" % (s, nm))   # noqa: E731
        for nm in _FUNCS:
            if nm != "create":
                f(nm).argtypes = [vp]
        f("create").restype = vp
        f("problem").restype = vp
        f("last_error").restype = C.c_char_p
        f("destroy").restype = None
        f("set_message_handlers").argtypes = [vp, vp, vp]
        f("set_message_handlers").restype = None
        f("set_device").argtypes = [vp, i]
        f("read").argtypes = [vp, C.c_char_p]
        f("open_document").argtypes = [vp, C.c_char_p]
        f("get_nodes").argtypes = [vp, dptr, dptr, dptr, iptr]
        f("get_elements").argtypes = [vp, iptr, iptr]
        f("get_conductors").argtypes = [vp, dptr, dptr]
        f("get_header").argtypes = [vp, dptr]
        f("get_block_label").argtypes = [vp, i, dptr]
        f("get_block_prop").argtypes = [vp, i, dptr]
        f("geometry_counts").argtypes = [vp, iptr]
        f("get_geometry_points").argtypes = [vp, dptr, dptr, iptr]
        f("get_geometry_segments").argtypes = [vp, iptr, iptr]
        f("get_geometry_arcs").argtypes = [vp, iptr, dptr, iptr]
        f("select_block_label").argtypes = [vp, d, d]
        f("toggle_label").argtypes = [vp, i]
        f("toggle_group").argtypes = [vp, i]
        f("get_selection").argtypes = [vp, ubptr]
        f("set_smoothing").argtypes = [vp, i]
        f("block_integral").argtypes = [vp, i, dptr]
        f("get_point_values").argtypes = [vp, d, d, dptr]
        f("get_point_values_batch").argtypes = [vp, i, dptr, dptr, iptr, dptr]
        f("add_contour_point").argtypes = [vp, d, d]
        f("add_contour_point_from_node").argtypes = [vp, d, d]
        f("bend_contour").argtypes = [vp, d, d]
        f("get_contour").argtypes = [vp, dptr, dptr]
        f("line_integral").argtypes = [vp, i, dptr]
        f("plot_bounds").argtypes = [vp, dptr]
    _lib = L
    return L


class _PProc:
    _name = ""
    _problem_class = None

    def __init__(self, device: int = 0, quiet: bool = False):
        load_library()
        self._h = C.c_void_p(self._f("create")())
        self._f("set_device")(self._h, device)
        if quiet:   # messages stay in last_error()
            self._cb = C.CFUNCTYPE(C.c_int, C.c_char_p)(lambda fmt: 0)
            self._f("set_message_handlers")(self._h, C.cast(self._cb, C.c_void_p), C.cast(self._cb, C.c_void_p))

    def _f(self, nm):
        return getattr(_lib, "xfemm_%s_%s" % (self._name, nm))

    def close(self):
        if getattr(self, "_h", None):
            self._f("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self) -> str:
        return self._f("last_error")(self._h).decode()

    def read(self, path: str) -> bool:
        """The file into host memory; False with last_error() on a bad file."""
        return bool(self._f("read")(self._h, str(path).encode()))

    def open(self, path: str) -> bool:
        """OpenDocument: read(), then the problem on the device."""
        return bool(self._f("open_document")(self._h, str(path).encode()))

    @property
    def NumNodes(self) -> int:
        return self._f("num_nodes")(self._h)

    @property
    def NumEls(self) -> int:
        return self._f("num_elements")(self._h)

    def nodes(self):
        """x, y (the problem's length units), the potential and the Q mark of every node."""
        n = self.NumNodes
        x, y, V = np.zeros(n), np.zeros(n), np.zeros(n)
        Q = np.zeros(n, np.int32)
        self._f("get_nodes")(self._h, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), V.ctypes.data_as(dptr),
                             Q.ctypes.data_as(iptr))
        return x, y, V, Q

    def elements(self):
        ne = self.NumEls
        p, lbl = np.zeros((ne, 3), np.int32), np.zeros(ne, np.int32)
        self._f("get_elements")(self._h, p.ctypes.data_as(iptr), lbl.ctypes.data_as(iptr))
        return p, lbl

    def conductors(self):
        """(V, q) of the file's conductor lines."""
        n = max(0, self._f("num_conductors")(self._h))
        V, q = np.zeros(max(1, n)), np.zeros(max(1, n))
        self._f("get_conductors")(self._h, V.ctypes.data_as(dptr), q.ctypes.data_as(dptr))
        return V[:n], q[:n]

    def header(self) -> dict:
        o = np.zeros(8)
        self._f("get_header")(self._h, o.ctypes.data_as(dptr))
        return dict(precision=o[0], depth=o[1], length_units=int(o[2]), problem_type=int(o[3]), ext_zo=o[4],
                    ext_ro=o[5], ext_ri=o[6], dt=o[7],
                    n_line_props=self._f("num_line_props")(self._h), n_node_props=self._f("num_node_props")(self._h),
                    n_block_props=self._f("num_block_props")(self._h),
                    n_block_labels=self._f("num_block_labels")(self._h))

    def labels(self) -> list:
        out = []
        for k in range(self._f("num_block_labels")(self._h)):
            o = np.zeros(6)
            self._f("get_block_label")(self._h, k, o.ctypes.data_as(dptr))
            out.append(dict(x=o[0], y=o[1], block=int(o[2]), group=int(o[3]), is_external=int(o[4]),
                            is_default=int(o[5])))
        return out

    def blocks(self) -> list:
        out = []
        for k in range(self._f("num_block_props")(self._h)):
            o = np.zeros(5)
            self._f("get_block_prop")(self._h, k, o.ctypes.data_as(dptr))
            out.append(dict(kx=o[0], ky=o[1], kt=o[2], qv=o[3], n_tk=int(o[4])))
        return out

    def geometry(self) -> dict:
        """The file's input geometry, as kernels.Contour.add_point_from_node takes it."""
        c = np.zeros(4, np.int32)
        self._f("geometry_counts")(self._h, c.ctypes.data_as(iptr))
        n, ns, na = int(c[0]), int(c[1]), int(c[2])
        x, y = np.zeros(max(1, n)), np.zeros(max(1, n))
        seg, arc = np.zeros((max(1, ns), 2), np.int32), np.zeros((max(1, na), 2), np.int32)
        lm = np.zeros((max(1, na), 2))
        self._f("get_geometry_points")(self._h, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr), None)
        self._f("get_geometry_segments")(self._h, seg.ctypes.data_as(iptr), None)
        self._f("get_geometry_arcs")(self._h, arc.ctypes.data_as(iptr), lm.ctypes.data_as(dptr), None)
        return dict(points=np.stack([x[:n], y[:n]], axis=1), segments=seg[:ns], arcs=arc[:na],
                    arc_length=lm[:na, 0].copy(), arc_maxside=lm[:na, 1].copy(), n_holes=int(c[3]))

    # --- selection, smoothing ---------------------------------------------------
    def clear_selection(self):
        self._f("clear_selection")(self._h)

    def select_block_label(self, x: float, y: float) -> bool:
        return bool(self._f("select_block_label")(self._h, x, y))

    def toggle_label(self, k: int) -> bool:
        return bool(self._f("toggle_label")(self._h, k))

    def toggle_group(self, g: int) -> bool:
        return bool(self._f("toggle_group")(self._h, g))

    def selection(self) -> np.ndarray:
        s = np.zeros(max(1, self._f("num_block_labels")(self._h)), np.uint8)
        self._f("get_selection")(self._h, s.ctypes.data_as(ubptr))
        return s[:self._f("num_block_labels")(self._h)]

    def set_smoothing(self, on: bool):
        self._f("set_smoothing")(self._h, int(bool(on)))

    def _ok(self, rc):
        if not rc:
            raise kernels.XfkError(self.last_error())

    # --- results ----------------------------------------------------------------
    def block_integral(self, kind: int) -> complex:
        o = np.zeros(2)
        self._ok(self._f("block_integral")(self._h, int(kind), o.ctypes.data_as(dptr)))
        return complex(o[0], o[1])

    def point_values(self, x: float, y: float):
        """The 8 values at one point, or None when no element holds it."""
        o = np.zeros(8)
        return o if self._f("get_point_values")(self._h, float(x), float(y), o.ctypes.data_as(dptr)) else None

    def point_values_batch(self, x, y) -> dict:
        x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        y = np.ascontiguousarray(np.atleast_1d(y), dtype=np.float64)
        n = len(x)
        el, o = np.zeros(max(1, n), np.int32), np.zeros((max(1, n), 8))
        self._ok(self._f("get_point_values_batch")(self._h, n, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr),
                                                    el.ctypes.data_as(iptr), o.ctypes.data_as(dptr)))
        return {"elem": el[:n], "raw": o[:n]}

    def add_contour_point(self, x: float, y: float):
        self._f("add_contour_point")(self._h, float(x), float(y))

    def add_contour_point_from_node(self, x: float, y: float):
        self._ok(self._f("add_contour_point_from_node")(self._h, float(x), float(y)))

    def bend_contour(self, angle: float, step: float = 1.0):
        self._f("bend_contour")(self._h, float(angle), float(step))

    def clear_contour(self):
        self._f("clear_contour")(self._h)

    def contour(self) -> np.ndarray:
        n = self._f("num_contour_points")(self._h)
        x, y = np.zeros(max(1, n)), np.zeros(max(1, n))
        self._f("get_contour")(self._h, x.ctypes.data_as(dptr), y.ctypes.data_as(dptr))
        return np.stack([x[:n], y[:n]], axis=1)

    def line_integral(self, kind: int) -> complex:
        o = np.zeros(2)
        self._ok(self._f("line_integral")(self._h, int(kind), o.ctypes.data_as(dptr)))
        return complex(o[0], o[1])

    def plot_bounds(self) -> np.ndarray:
        o = np.zeros(6)
        self._ok(self._f("plot_bounds")(self._h, o.ctypes.data_as(dptr)))
        return o.reshape(3, 2)

    def has_multiply_defined_labels(self) -> bool:
        return bool(self._f("has_multiply_defined_labels")(self._h))

    def problem(self):
        """The opened problem as its kernels class, around the live handle
        (owned by this post-processor: valid until its next open or its end)."""
        h = self._f("problem")(self._h)
        if not h:
            raise RuntimeError("no document is open (open first)")
        kernels.load_library()
        cls = type("Opened" + self._problem_class.__name__, (_Borrowed, self._problem_class), {})
        P = cls.__new__(cls)
        P._h = C.c_void_p(h)
        P._owner = self
        P.n_nodes = P.n_rows = self.NumNodes
        P.n_elems = self.NumEls
        P.n_conductors = max(0, self._f("num_conductors")(self._h))
        P.n_labels = self._f("num_block_labels")(self._h)
        P.result = None
        return P


class EPProc(_PProc):
    """The reference's epproc over the MI355X post-processing: a .res in."""
    _name = "epproc"
    _problem_class = kernels.ElectrostaticProblem


class HPProc(_PProc):
    """The reference's hpproc over the MI355X post-processing: an .anh in."""
    _name = "hpproc"
    _problem_class = kernels.HeatFlowProblem
