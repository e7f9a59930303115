"""Device objects over the C-ABI: meshes, function spaces, matrices, vectors
and the Krylov solve, one GPU per process.

These play the role of dolfin's Mesh/FunctionSpace/PETScMatrix/PETScVector/
PETScKrylovSolver for the hot path of FenicsSolver/SolverBase.py:592-672.
Everything here runs on the MI355X through libfsamd.so; nothing is computed
on the host and nothing falls back to it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib as L
from ._lib import BackendError  # noqa: F401  (re-export)


def init(device_id=0):
    L.check(L.load().fs_init(int(device_id)), "fs_init")


def device_count():
    n = C.c_int(0)
    L.load().fs_device_count(C.byref(n))
    return n.value


def device_info():
    name = C.create_string_buffer(256)
    cus = C.c_int(0)
    mem = C.c_int64(0)
    L.check(L.load().fs_device_info(name, 256, C.byref(cus), C.byref(mem)), "fs_device_info")
    return {"name": name.value.decode(), "compute_units": cus.value, "hbm_bytes": mem.value}


def synchronize():
    L.check(L.load().fs_device_synchronize(), "fs_device_synchronize")


def profile_marker(phase):
    """An empty, named launch (k_profile_marker) between the legs of a traced command: the n-th one opens phase n of
    tools/summarize_profiles.py."""
    L.check(L.load().fs_profile_marker(int(phase)), "fs_profile_marker")


def memory_info():
    """Bytes of device memory the library holds: in use by live objects / idle in its block cache."""
    live, cached = C.c_int64(0), C.c_int64(0)
    L.check(L.load().fs_memory_info(C.byref(live), C.byref(cached)), "fs_memory_info")
    return {"live_bytes": live.value, "cached_bytes": cached.value}


def trim_memory():
    """Return the idle blocks of the cache to the driver."""
    L.check(L.load().fs_memory_trim(), "fs_memory_trim")


class _Handle:
    _destroy = None
    _serials = [0]

    def __init__(self):
        self.h = C.c_void_p()
        _Handle._serials[0] += 1
        self.serial = _Handle._serials[0]      # never reused (id() is): what caches keyed on a device object compare

    def close(self):
        if self.h is not None and self.h.value:
            getattr(L.load(), self._destroy)(self.h)
            self.h = C.c_void_p()

    def __del__(self):  # best effort
        try:
            self.close()
        except Exception:
            pass


class DeviceMesh(_Handle):
    """Tetrahedral mesh resident in HBM (dolfin.Mesh, SolverBase.py:203-258)."""
    _destroy = "fs_mesh_destroy"

    def __init__(self, coords=None, cells=None, n_owned=None, global_ids=None):
        super().__init__()
        if coords is None:
            return
        coords = L.f64(coords)
        cells = L.i32(cells)
        if coords.ndim != 2 or cells.ndim != 2:
            raise BackendError("DeviceMesh: coords must be [nv,gdim], cells [nc,verts]")
        nv = coords.shape[0]
        if n_owned is None:
            n_owned = nv
        self._keep = (coords, cells)
        L.check(L.load().fs_mesh_create(coords.shape[1], nv, L.p_f64(coords), cells.shape[0], L.p_i32(cells),
                                        cells.shape[1], int(n_owned), C.byref(self.h)), "fs_mesh_create")
        self._keep = None
        if global_ids is not None:
            g = L.i64(global_ids)
            if g.shape != (nv,):
                raise BackendError("DeviceMesh: global_ids must have one entry per local vertex")
            L.check(L.load().fs_mesh_set_global_ids(self.h, L.p_i64(g)), "fs_mesh_set_global_ids")

    @classmethod
    def box(cls, nx, ny, nz, p0=(0.0, 0.0, 0.0), p1=(1.0, 1.0, 1.0), zplanes=None):
        """Slab [zplanes[0], zplanes[1]) of BoxMesh(p0,p1,nx,ny,nz) generated on the device."""
        m = cls()
        if zplanes is None:
            zplanes = (0, nz + 1)
        a = L.f64(p0)
        b = L.f64(p1)
        L.check(L.load().fs_mesh_create_box(int(nx), int(ny), int(nz), L.p_f64(a), L.p_f64(b), int(zplanes[0]),
                                            int(zplanes[1]), C.byref(m.h)), "fs_mesh_create_box")
        return m

    @classmethod
    def renumbered(cls, coords, cells):
        """A tetrahedral mesh that arrives in FILE order, uploaded once and built on the device in the locality order of
        fs_mesh_locality_order (global vertex ids = the file's numbers).  Returns (mesh, vertex_order, cell_order):
        vertex_order[k] / cell_order[c] = file number of device vertex k / device cell c."""
        co, ce = L.f64(coords), L.i32(cells)
        if co.ndim != 2 or co.shape[1] != 3 or ce.ndim != 2 or ce.shape[1] != 4:
            raise BackendError("DeviceMesh.renumbered: coords [nv,3] and cells [nc,4]")
        m = cls()
        vo = np.empty(co.shape[0], dtype=np.int32)
        cord = np.empty(ce.shape[0], dtype=np.int32)
        L.check(L.load().fs_mesh_create_renumbered(co.shape[0], L.p_f64(co), ce.shape[0], L.p_i32(ce), L.p_i32(vo), L.p_i32(cord),
                                                   C.byref(m.h)), "fs_mesh_create_renumbered")
        return m, vo, cord

    def info(self):
        nv, nc, no = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.load().fs_mesh_info(self.h, C.byref(nv), C.byref(nc), C.byref(no)), "fs_mesh_info")
        return nv.value, nc.value, no.value

    def get(self, want_coords=True, want_cells=True, want_gids=True):
        nv, nc, _ = self.info()
        xyz = np.empty((nv, 3)) if want_coords else None
        cells = np.empty((nc, 4), dtype=np.int32) if want_cells else None
        gid = np.empty(nv, dtype=np.int64) if want_gids else None
        L.check(L.load().fs_mesh_get(self.h, L.p_f64(xyz), L.p_i32(cells), L.p_i64(gid)), "fs_mesh_get")
        return xyz, cells, gid


def locality_order(coords, cells):
    """(vertex_order, cell_order): the order in which to upload the vertices and cells of a mesh that arrives in file order
    (Morton curve of the coordinates, computed on the device; fs_mesh_locality_order).  vertex_order[k] = old id of new
    vertex k."""
    co, ce = L.f64(coords), L.i32(cells)
    vo = np.empty(co.shape[0], dtype=np.int32)
    cord = np.empty(ce.shape[0], dtype=np.int32)
    L.check(L.load().fs_mesh_locality_order(co.shape[1], co.shape[0], L.p_f64(co), ce.shape[0], L.p_i32(ce), ce.shape[1],
                                            L.p_i32(vo), L.p_i32(cord)), "fs_mesh_locality_order")
    return vo, cord


class DeviceSpace(_Handle):
    """CG1 (scalar or 3-vector) space + sparsity (FunctionSpace, SolverBase.py:260-275)."""
    _destroy = "fs_space_destroy"

    def __init__(self, mesh, ncomp=1, degree=1, coupled_pairs=None):
        """coupled_pairs [n,2]: extra node couplings of the sparsity pattern (interior-facet integrals)."""
        super().__init__()
        self.mesh = mesh
        self.ncomp = int(ncomp)
        if coupled_pairs is None:
            L.check(L.load().fs_space_create(mesh.h, 0, int(degree), int(ncomp), C.byref(self.h)), "fs_space_create")
        else:
            pairs = L.i32(coupled_pairs).reshape(-1, 2)
            L.check(L.load().fs_space_create_coupled(mesh.h, 0, int(degree), int(ncomp), pairs.shape[0], L.p_i32(pairs),
                                                     C.byref(self.h)), "fs_space_create_coupled")
        self.facet_coupled = coupled_pairs is not None
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.load().fs_space_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "fs_space_info")
        self.n_local, self.n_owned, self.nnz, self.sell_entries = a.value, b.value, c.value, d.value
        L.check(L.load().fs_space_format_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "fs_space_format_info")
        self.n_slices, self.n_dia_slices, self.spmv_matrix_bytes = a.value, b.value, c.value
        self.degree = int(degree)

    def edges(self):
        """CG2: [n_edges,2] vertex pairs of the edge nodes (dof = n_vertices + row index)."""
        ne = C.c_int64(0)
        L.check(L.load().fs_space_get_edges(self.h, C.byref(ne), None), "fs_space_get_edges")
        out = np.empty((ne.value, 2), dtype=np.int32)
        if ne.value:
            L.check(L.load().fs_space_get_edges(self.h, C.byref(ne), L.p_i32(out)), "fs_space_get_edges")
        return out

    def set_halo(self, neighbors, send_lists, recv_counts, recv_lists=None):
        """neighbors: ranks; send_lists: per neighbour array of owned local dofs; recv_counts: ghosts per neighbour;
        recv_lists: per neighbour the local ghost dof of every received value (None: ghosts grouped by neighbour)."""
        if getattr(self, "_p2p", False):
            self.enable_p2p_halo(False)
        nb = L.i32(neighbors)
        sc = L.i64([len(s) for s in send_lists])
        si = L.i32(np.concatenate([np.asarray(s, dtype=np.int32) for s in send_lists]) if len(send_lists) else [])
        rc = L.i64(recv_counts)
        if recv_lists is None:
            L.check(L.load().fs_space_set_halo(self.h, len(nb), L.p_i32(nb), L.p_i64(sc), L.p_i32(si), L.p_i64(rc)),
                    "fs_space_set_halo")
        else:
            ri = L.i32(np.concatenate([np.asarray(r, dtype=np.int32) for r in recv_lists]) if len(recv_lists) else [])
            L.check(L.load().fs_space_set_halo_indexed(self.h, len(nb), L.p_i32(nb), L.p_i64(sc), L.p_i32(si), L.p_i64(rc),
                                                       L.p_i32(ri)), "fs_space_set_halo_indexed")
        # The peer-to-peer exchange (29 instead of 55 us per CG iteration at 1 M rows per rank with the rank its own neighbour,
        # profiles/*_p2p_self_halo_timings.txt) is OPT-IN until it has crossed a device boundary on hardware (round 5):
        # FS_HALO_P2P=auto tries it - the set-up ends with a self-test whose verdict all ranks agree on, and a node where the
        # mappings cannot be made falls back to RCCL on EVERY rank, here; FS_HALO_P2P=1: a failed set-up is an error instead of a
        # fall-back; unset / 0: RCCL send / recv.  bench.py tries every transport explicitly and times the fastest that reproduces
        # the RCCL field.
        mode = os.environ.get("FS_HALO_P2P", "0")
        if _comm_up and mode != "0" and comm_info()[0] > 1:
            try:
                self.enable_p2p_halo(True)
            except L.BackendError as e:
                if mode == "1":
                    raise
                import logging
                logging.getLogger("fenicssolver_amd").info("peer-to-peer halo exchange not available (%s): RCCL send / recv", str(e)[:160])

    def enable_p2p_halo(self, on=True):
        """Ghost refresh by direct stores into the neighbours' memory (hipIpc mappings, one node) instead of RCCL send / recv.
        COLLECTIVE: every rank of the communicator calls it for its space, in the same order (also to turn it off).
        Environment FS_HALO_P2P=auto / 1 turns it on for every halo plan set while a communicator of more than one rank is up."""
        self._p2p = False
        L.check(L.load().fs_space_enable_p2p_halo(self.h, 1 if on else 0), "fs_space_enable_p2p_halo")
        self._p2p = bool(on)


class DeviceVector(_Handle):
    _destroy = "fs_vector_destroy"

    def __init__(self, n, values=None):
        super().__init__()
        self.n = int(n)
        L.check(L.load().fs_vector_create(self.n, C.byref(self.h)), "fs_vector_create")
        if values is not None:
            self.set(values)

    def set(self, values):
        v = L.f64(values).ravel()
        if v.size != self.n:
            raise BackendError("DeviceVector.set: %d values for a vector of %d" % (v.size, self.n))
        L.check(L.load().fs_vector_set(self.h, L.p_f64(v), self.n), "fs_vector_set")

    def get(self, n=None):
        n = self.n if n is None else int(n)
        out = np.empty(n)
        L.check(L.load().fs_vector_get(self.h, L.p_f64(out), n), "fs_vector_get")
        return out

    def fill(self, a):
        L.check(L.load().fs_vector_fill(self.h, float(a)), "fs_vector_fill")

    def copy_from(self, src, n=None):
        n = min(self.n, src.n) if n is None else int(n)
        L.check(L.load().fs_vector_copy(self.h, src.h, n), "fs_vector_copy")

    def axpy(self, a, x):
        L.check(L.load().fs_vector_axpy(self.h, float(a), x.h), "fs_vector_axpy")

    def add_entries(self, idx, vals):
        i, v = L.i32(idx).ravel(), L.f64(vals).ravel()
        L.check(L.load().fs_vector_add_entries(self.h, i.size, L.p_i32(i), L.p_f64(v)), "fs_vector_add_entries")

    def assign_entries(self, dst_nodes, src_nodes, block=1):
        """self[dst*block + c] = self[src*block + c] (the slaves of a periodic constraint take their masters' values)."""
        d, sr = L.i32(dst_nodes).ravel(), L.i32(src_nodes).ravel()
        L.check(L.load().fs_vector_assign_entries(self.h, d.size, L.p_i32(d), L.p_i32(sr), int(block)), "fs_vector_assign_entries")

    def dot(self, y):
        r = C.c_double(0.0)
        L.check(L.load().fs_vector_dot(self.h, y.h, C.byref(r)), "fs_vector_dot")
        return r.value

    def rotate_nodes(self, frames):
        """self <- H self with the node reflectors of a ContactFrames (H is its own inverse: the same call leads back)."""
        L.check(L.load().fs_vector_rotate_nodes(self.h, frames.h), "fs_vector_rotate_nodes")


def _coef(spec, keep):
    """spec: None | number | ('cell', array) | ('nodal', array) | ('tensor', 3x3) | ('cell_tensor', [n_cells,3,3])."""
    c = L.fs_coef()
    if spec is None:
        c.mode = L.FS_COEF_NONE
    elif isinstance(spec, tuple):
        kind, arr = spec
        if kind == "tensor":
            c.mode = L.FS_COEF_TENSOR
            t = L.f64(arr).reshape(9)
            for i in range(9):
                c.tensor[i] = t[i]
        elif kind == "cell_qp":              # [n_cells, 14]: the coefficient at the points of the degree-5 rule (CG2 spaces)
            a = L.f64(np.ascontiguousarray(arr).reshape(-1, 14))
            keep.append(a)
            c.mode = L.FS_COEF_CELL_QP
            c.data = L.p_f64(a)
        elif kind == "cell_tensor":          # [n_cells, 3, 3]
            a = L.f64(np.ascontiguousarray(arr).reshape(-1, 9))
            keep.append(a)
            c.mode = L.FS_COEF_CELL_TENSOR
            c.data = L.p_f64(a)
        else:
            a = L.f64(arr).ravel()
            keep.append(a)
            c.mode = L.FS_COEF_CELL if kind == "cell" else L.FS_COEF_NODAL
            c.data = L.p_f64(a)
    else:
        c.mode = L.FS_COEF_CONST
        c.value = float(spec)
    return c


def _bilinear_form(keep, stiffness=None, mass=None, lame=None, advection=None, advection_scale=1.0, supg_pe=0.0):
    f = L.fs_bilinear_form()
    f.stiffness = _coef(stiffness, keep)
    f.mass = _coef(mass, keep)
    if advection is not None:
        v = L.f64(advection)
        if v.size == 3:
            f.advection.mode = L.FS_COEF_CONST
            for i in range(3):
                f.advection.tensor[i] = float(v.ravel()[i])
        elif v.ndim == 3:           # [n_cells, d+1, 3]: one velocity per cell and test function (fem.row_velocities)
            v = L.f64(np.ascontiguousarray(v).reshape(-1, 3))
            keep.append(v)
            f.advection.mode = L.FS_COEF_CELL_ROW
            f.advection.data = L.p_f64(v)
        else:
            v = L.f64(v.reshape(-1, 3))
            keep.append(v)
            f.advection.mode = L.FS_COEF_CELL
            f.advection.data = L.p_f64(v)
        f.advection_scale = float(advection_scale)
        f.supg_pe = float(supg_pe)
    if lame is not None:
        if _is_cell_lame(lame):
            f.lame.mode = L.FS_COEF_CELL_LAME              # ('cell', [n_cells, 2]): one (mu, lambda) pair per cell
            f.lame.data = L.p_f64(_lame_cells(lame, keep))
        else:
            f.lame_mu, f.lame_lambda = float(lame[0]), float(lame[1])
    return f


def _is_cell_lame(lame):
    return isinstance(lame, tuple) and len(lame) == 2 and isinstance(lame[0], str)


def _lame_cells(lame, keep, n_cells=None):
    kind, arr = lame
    if kind != "cell":
        raise BackendError("Lame parameters: (mu, lambda) numbers or ('cell', array[n_cells, 2]), got kind %r" % (kind,))
    a = np.ascontiguousarray(arr, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 2 or (n_cells is not None and a.shape[0] != n_cells):
        raise BackendError("per-cell Lame parameters must be an array [%s, 2], got shape %s" % (n_cells, a.shape))
    keep.append(a)
    return a


def apply_operator(space, x, y, stiffness=None, mass=None, advection=None, advection_scale=1.0, supg_pe=0.0, reps=0):
    """Matrix-free y = K(form) x on a scalar CG1 or CG2 space over tetrahedra (no matrix is formed, no Dirichlet rows; CG2: constant
    or per-cell scalar coefficients, no advection).
    reps > 1: also returns the mean milliseconds of reps products timed with HIP events."""
    keep = []
    f = _bilinear_form(keep, stiffness, mass, None, advection, advection_scale, supg_pe)
    ms = C.c_double(0.0)
    L.check(L.load().fs_operator_apply(space.h, C.byref(f), x.h, y.h, int(reps), C.byref(ms)), "fs_operator_apply")
    return ms.value if reps > 1 else None


class DeviceMatrix(_Handle):
    """SELL-64 matrix on a space's pattern (PETSc AIJ behind dolfin.assemble)."""
    _destroy = "fs_matrix_destroy"

    def __init__(self, space):
        super().__init__()
        self.space = space
        L.check(L.load().fs_matrix_create(space.h, C.byref(self.h)), "fs_matrix_create")

    def assemble(self, stiffness=None, mass=None, lame=None, advection=None, advection_scale=1.0, add=False, supg_pe=0.0):
        """advection: constant velocity (3 numbers) or per-cell array [n_cells,3]; supg_pe > 0: SUPG test function
        q + tau (v . grad q) on the advection and mass terms."""
        keep = []
        if _is_cell_lame(lame):
            lame = ("cell", _lame_cells(lame, keep, self.space.mesh.info()[1]))
        f = _bilinear_form(keep, stiffness, mass, lame, advection, advection_scale, supg_pe)
        L.check(L.load().fs_assemble_matrix(self.h, C.byref(f), 1 if add else 0), "fs_assemble_matrix")

    def assemble_anisotropic(self, material, mass=None, add=False):
        """self (+)= int eps(v) : C : eps(u) dx + mass u.v on a vector CG1 space (fs_assemble_anisotropic).  material: an
        AnisotropicMaterial or a tuple (table[n, 6, 6] in library order, material_of_cell or None, frames or None) in device cell
        order; mass: None, a number or ('cell', array[n_cells])."""
        keep = []
        nc = self.space.mesh.info()[1]
        m = _aniso_material(material, nc, keep)
        if isinstance(mass, tuple):
            if mass[0] != "cell" or np.shape(mass[1]) != (nc,):
                raise BackendError("assemble_anisotropic: mass is a number or ('cell', array[%d]), got (%r, shape %s)"
                                   % (nc, mass[0], np.shape(mass[1])))
        mc = _coef(mass, keep)
        L.check(L.load().fs_assemble_anisotropic(self.h, C.byref(m), C.byref(mc), 1 if add else 0), "fs_assemble_anisotropic")

    def assemble_geometric(self, lame, u, cell_stress=False):
        """The geometric stiffness K_G of the linear-elastic stress of the displacement u (DeviceVector of the space's dofs) on a
        vector CG1 space (fs_assemble_geometric_stiffness): every node-pair block is s I.  lame as assemble(lame=...): (mu, lambda)
        numbers or ('cell', array[n_cells, 2]) in device cell order.  cell_stress=True: returns the stress per cell, array
        [n_cells, 6] (xx, yy, zz, xy, xz, yz) or [n_cells, 4] (xx, yy, zz, xy) in plane strain, device cell order; else None."""
        keep = []
        mu = lm = 0.0
        cells = None
        nc = self.space.mesh.info()[1]
        if _is_cell_lame(lame):
            cells = L.p_f64(_lame_cells(lame, keep, nc))
        else:
            mu, lm = float(lame[0]), float(lame[1])
        sig = np.empty((nc, 6 if self.space.ncomp == 3 else 4)) if cell_stress else None
        L.check(L.load().fs_assemble_geometric_stiffness(self.space.h, mu, lm, cells, u.h, self.h, L.p_f64(sig)),
                "fs_assemble_geometric_stiffness")
        return sig

    def add_facet_mass(self, tri, h):
        tri = L.i32(tri)
        tri = tri.reshape(-1, 3) if tri.ndim == 1 else tri       # [nf,3] triangles (3-D) or [nf,2] edges (2-D)
        h = L.f64(np.broadcast_to(h, (tri.shape[0],)))
        L.check(L.load().fs_assemble_facet_matrix(self.h, tri.shape[0], L.p_i32(tri), L.p_f64(h)),
                "fs_assemble_facet_matrix")

    def add_interior_penalty(self, facet_cells, coefficient):
        """+= coefficient * avg(h)^2 jump(grad u, n) jump(grad v, n) dS over the interior facets [nf,2] (cell pairs)."""
        fc = L.i32(facet_cells).reshape(-1, 2)
        L.check(L.load().fs_assemble_interior_penalty(self.h, fc.shape[0], L.p_i32(fc), float(coefficient)),
                "fs_assemble_interior_penalty")

    def axpy(self, a, X):
        L.check(L.load().fs_matrix_axpy(self.h, float(a), X.h), "fs_matrix_axpy")

    def tie_nodes(self, b, slaves, masters):
        """Fold the periodic constraint u[slaves] = u[masters] into the assembled system (and b, which may be None)."""
        sl, ma = L.i32(slaves).ravel(), L.i32(masters).ravel()
        L.check(L.load().fs_matrix_tie_nodes(self.h, b.h if b is not None else None, sl.size, L.p_i32(sl), L.p_i32(ma)),
                "fs_matrix_tie_nodes")

    def copy_from(self, src):
        """self = src (same space), on the library's stream."""
        L.check(L.load().fs_matrix_copy(self.h, src.h), "fs_matrix_copy")

    def zero(self):
        L.check(L.load().fs_matrix_zero(self.h), "fs_matrix_zero")

    def rotate_nodes(self, frames):
        """self <- H self H in place with the node reflectors of a ContactFrames (fs_matrix_rotate_nodes): block sizes 2 and 3, the
        pattern unchanged, blocks with neither node framed not written."""
        L.check(L.load().fs_matrix_rotate_nodes(self.h, frames.h), "fs_matrix_rotate_nodes")

    def apply_dirichlet(self, b, dofs, vals, symmetric=True):
        dofs = L.i32(dofs).ravel()
        vals = L.f64(np.broadcast_to(vals, dofs.shape))
        L.check(L.load().fs_apply_dirichlet(self.h, b.h if b is not None else None, dofs.size, L.p_i32(dofs),
                                            L.p_f64(vals), 1 if symmetric else 0), "fs_apply_dirichlet")

    def to_csr(self):
        """(rowptr, colidx, vals) sorted-column CSR copy on the host."""
        nr, ncol, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.load().fs_matrix_info(self.h, C.byref(nr), C.byref(ncol), C.byref(nnz)), "fs_matrix_info")
        rp = np.empty(nr.value + 1, dtype=np.int32)
        ci = np.empty(nnz.value, dtype=np.int32)
        va = np.empty(nnz.value)
        L.check(L.load().fs_matrix_get_csr(self.h, L.p_i32(rp), L.p_i32(ci), L.p_f64(va)), "fs_matrix_get_csr")
        return rp, ci, va, (nr.value, ncol.value)

    def spmv(self, x, y):
        L.check(L.load().fs_spmv(self.h, x.h, y.h), "fs_spmv")

    def spmv_dictionary(self, x, y):
        """y = A x through the row-dictionary product where the rows repeat; returns the number of distinct rows used (0: streaming)."""
        nc = C.c_int(0)
        L.check(L.load().fs_spmv_dictionary(self.h, x.h, y.h, C.byref(nc)), "fs_spmv_dictionary")
        return nc.value

    def spmv_benchmark(self, x, y, reps=20):
        ms = C.c_double(0.0)
        L.check(L.load().fs_spmv_benchmark(self.h, x.h, y.h, int(reps), C.byref(ms)), "fs_spmv_benchmark")
        return ms.value


class ContactFrames(_Handle):
    """The node frames and the active-set state of frictionless contact / sliding supports on a vector CG1 space (fs_contact_t).
    nodes: ascending node ids; normals [n, d] (normalised by the library); values [n]: the clearance along the normal of a contact
    node, the prescribed normal displacement of a bilateral one; bilateral [n]: sliding supports, always active; active [n]: the
    first active set.  normal_dofs: d * node + (d - 1), the dof that holds sigma n . u in the rotated unknowns."""
    _destroy = "fs_contact_destroy"

    def __init__(self, space, nodes, normals, values=0.0, bilateral=False, active=True):
        super().__init__()
        self.space = space
        nodes = L.i32(nodes).ravel()
        d = space.ncomp
        nrm = L.f64(normals).reshape(-1, d)
        if nrm.shape[0] != nodes.size:
            raise BackendError("ContactFrames: %d normals for %d nodes" % (nrm.shape[0], nodes.size))
        self.nodes, self.n = nodes, nodes.size
        self.bilateral = L.i32(np.broadcast_to(np.asarray(bilateral, dtype=np.int32), nodes.shape))
        vals = L.f64(np.broadcast_to(values, nodes.shape))
        act = L.i32(np.broadcast_to(np.asarray(active, dtype=np.int32), nodes.shape))
        L.check(L.load().fs_contact_create(space.h, self.n, L.p_i32(nodes), L.p_f64(nrm), L.p_f64(vals), L.p_i32(self.bilateral),
                                           L.p_i32(act), C.byref(self.h)), "fs_contact_create")
        length = np.linalg.norm(nrm, axis=1)
        self.normals = nrm / length[:, None]
        self.values = vals.copy()
        self.sigma = np.where(self.normals[:, d - 1] < 0.0, 1.0, -1.0)
        self.normal_dofs = (d * nodes.astype(np.int64) + (d - 1)).astype(np.int32)

    def get(self):
        """(active flags, lambda, penetration) of the last contact_update (before the first: the first active set, zeros)."""
        act, lam, pen = np.empty(self.n, dtype=np.int32), np.empty(self.n), np.empty(self.n)
        L.check(L.load().fs_contact_get(self.h, L.p_i32(act), L.p_f64(lam), L.p_f64(pen)), "fs_contact_get")
        return act.astype(bool), lam, pen


def contact_update(state, Kprime, uprime, bprime):
    """One primal-dual active-set update (fs_contact_update) from the solution u' of the system constrained on the state's active
    set, with the unconstrained rotated K' and b'.  Returns (flags changed, flags active)."""
    counts = np.zeros(2, dtype=np.int32)
    L.check(L.load().fs_contact_update(state.h, Kprime.h, uprime.h, bprime.h, L.p_i32(counts)), "fs_contact_update")
    return int(counts[0]), int(counts[1])


def _velocity_coef(v, keep):
    """Constant velocity (3 numbers) or per-cell array [n_cells,3] -> fs_coef."""
    c = L.fs_coef()
    v = L.f64(v)
    if v.size == 3:
        c.mode = L.FS_COEF_CONST
        for i in range(3):
            c.tensor[i] = float(v.ravel()[i])
    else:
        v = L.f64(v.reshape(-1, 3))
        keep.append(v)
        c.mode = L.FS_COEF_CELL
        c.data = L.p_f64(v)
    return c


def assemble_facet_supg(space, A, b, facet_cell, facet_opposite, velocity, pe, g=None, h=None):
    """SUPG part of ds(i) terms: b_a += g area w_a, A_ab += h (area/3) w_a (b on the facet), w_a = tau (v . grad phi_a)."""
    fc = np.ascontiguousarray(facet_cell, dtype=np.int32)
    fo_ = np.ascontiguousarray(facet_opposite, dtype=np.int32)
    keep = []
    vel = _velocity_coef(velocity, keep)
    gg = None if g is None else np.ascontiguousarray(np.broadcast_to(np.asarray(g, dtype=np.float64), fc.shape))
    hh = None if h is None else np.ascontiguousarray(np.broadcast_to(np.asarray(h, dtype=np.float64), fc.shape))
    L.check(L.load().fs_assemble_facet_supg(space.h, A.h if A is not None else None, b.h if b is not None else None, len(fc),
                                            L.p_i32(fc), L.p_i32(fo_), L.p_f64(gg), L.p_f64(hh), C.byref(vel), float(pe)),
            "fs_assemble_facet_supg")


def assemble_vector(space, b, source=None, vector_value=None, div_coef=None, add=False, supg=None):
    """b (+)= int source q dx [+ int f.v dx + int div_coef div v dx on vector spaces]; supg = (velocity, Pe) adds
    int source tau (v . grad q) dx."""
    keep = []
    f = L.fs_linear_form()
    f.source = _coef(source, keep)
    f.div_coef = _coef(div_coef, keep)
    if supg is not None:
        f.supg_velocity = _velocity_coef(supg[0], keep)
        f.supg_pe = float(supg[1])
    if vector_value is not None:
        for i, x in enumerate(vector_value):         # 3 components (2 on triangular meshes)
            f.vector_value[i] = float(x)
    L.check(L.load().fs_assemble_vector(space.h, C.byref(f), b.h, 1 if add else 0), "fs_assemble_vector")


def assemble_facet_vector(space, b, tri, g):
    """b_a += int g phi_a ds over the facets tri[nf,3]; g scalar, [ncomp], [nf] or [nf,ncomp]."""
    tri = L.i32(tri)
    tri = tri.reshape(-1, 3) if tri.ndim == 1 else tri           # [nf,3] triangles (3-D) or [nf,2] edges (2-D)
    nf, nc = tri.shape[0], space.ncomp
    g = np.asarray(g, dtype=np.float64)
    if g.ndim == 0:
        g = np.full((nf, nc), float(g))
    elif g.ndim == 1 and nc > 1 and g.size == nc:
        g = np.broadcast_to(g[None, :], (nf, nc))
    elif g.ndim == 1:
        g = g.reshape(nf, 1) if nc == 1 else np.broadcast_to(g[:, None], (nf, nc))
    g = L.f64(g)
    if g.shape != (nf, nc):
        raise BackendError("assemble_facet_vector: g has shape %s, expected (%d,%d)" % (g.shape, nf, nc))
    L.check(L.load().fs_assemble_facet_vector(space.h, nf, L.p_i32(tri), L.p_f64(g), b.h),
            "fs_assemble_facet_vector")


def _same_device_mesh(field_space, p1_space, what):
    """A projection reads a field of one space cell by cell and loads another: both on ONE device mesh.  On several ranks a periodic
    space cuts its own part (its masters are extra ghosts), and an unconstrained space made BEFORE it on the same host mesh sits on
    another one (fem.FunctionSpace._make_parallel_device shares the periodic part only with spaces made after it)."""
    if field_space.mesh is not p1_space.mesh:
        raise BackendError("%s: the two spaces live on different device meshes (parts) of the same host mesh - on several ranks create "
                           "the periodic function space BEFORE the unconstrained spaces that share its mesh" % what)


def assemble_von_mises(disp_space, u, mu, lmbda, p1_space, b):
    """b_a = int sqrt(3/2 s:s) phi_a dx, s the deviator of sigma(u), on the scalar CG1 space of the same mesh.
    Per-cell material: mu = ('cell', array[n_cells, 2]) of (mu, lambda) pairs in device cell order, lmbda = None."""
    _same_device_mesh(disp_space, p1_space, "assemble_von_mises")
    if _is_cell_lame(mu):
        a = _lame_cells(mu, [], disp_space.mesh.info()[1])
        L.check(L.load().fs_assemble_von_mises_cells(disp_space.h, u.h, L.p_f64(a), p1_space.h, b.h), "fs_assemble_von_mises_cells")
        return
    L.check(L.load().fs_assemble_von_mises(disp_space.h, u.h, float(mu), float(lmbda), p1_space.h, b.h), "fs_assemble_von_mises")


class AnisotropicMaterial:
    """An anisotropic elastic material as the device layer takes it (fs_aniso_material): ``table`` [n, 6, 6] symmetric matrices in
    the library's tensor order (xx, yy, zz, xy, xz, yz) with engineering shears, ``material_of_cell`` [n_cells] table indices in
    device cell order (None: one material everywhere, or - with n == n_cells - one per cell) and ``frames`` [n_cells, 3, 3] rotations
    whose columns are the material axes in global coordinates (None: the global axes)."""

    def __init__(self, table, material_of_cell=None, frames=None):
        self.table, self.material_of_cell, self.frames = table, material_of_cell, frames


_ANISO_TRIU = np.triu_indices(6)


def _aniso_material(material, n_cells, keep):
    """fs_aniso_material of an AnisotropicMaterial or a tuple (table, material_of_cell, frames); wrong lengths: BackendError."""
    if isinstance(material, AnisotropicMaterial):
        material = (material.table, material.material_of_cell, material.frames)
    if not isinstance(material, (tuple, list)) or len(material) != 3:
        raise BackendError("anisotropic material: an AnisotropicMaterial or a tuple (table[n, 6, 6], material_of_cell or None, "
                           "frames or None) is expected, got %s" % type(material).__name__)
    table, index, frames = material
    D = np.asarray(table, dtype=np.float64)
    if D.ndim == 2:
        D = D[None]
    if D.ndim != 3 or D.shape[1:] != (6, 6) or D.shape[0] < 1:
        raise BackendError("anisotropic material: the table must be an array [n, 6, 6], got shape %s" % (D.shape,))
    if not np.array_equal(D, np.transpose(D, (0, 2, 1)), equal_nan=True):      # (entries that are not finite: the C call's check)
        raise BackendError("anisotropic material: a 6x6 matrix of the table is not symmetric")
    m = L.fs_aniso_material()
    tri = np.ascontiguousarray(D[:, _ANISO_TRIU[0], _ANISO_TRIU[1]])
    keep.append(tri)
    m.n_materials = D.shape[0]
    m.stiffness = L.p_f64(tri)
    if index is not None:
        idx = np.asarray(index)
        if idx.ndim != 1 or idx.shape[0] != n_cells or not np.issubdtype(idx.dtype, np.integer):
            raise BackendError("anisotropic material: material_of_cell must be an integer array [%d], got shape %s" % (n_cells, idx.shape))
        idx = L.i32(idx)
        keep.append(idx)
        m.material_of_cell = L.p_i32(idx)
    elif D.shape[0] not in (1, n_cells):
        raise BackendError("anisotropic material: without material_of_cell the table holds 1 material or one per cell (%d), got %d"
                           % (n_cells, D.shape[0]))
    if frames is not None:
        R = np.ascontiguousarray(frames, dtype=np.float64)
        if R.shape != (n_cells, 3, 3) and R.shape != (n_cells, 9):
            raise BackendError("anisotropic material: frames must be an array [%d, 3, 3], got shape %s" % (n_cells, R.shape))
        keep.append(R)
        m.frame = L.p_f64(R)
    return m


def _aniso_eigenstrain(eigenstrain, space, n_cells):
    if eigenstrain is None:
        return None
    ne = 6 if space.ncomp == 3 else 4
    e = np.ascontiguousarray(eigenstrain, dtype=np.float64)
    if e.shape != (n_cells, ne):
        raise BackendError("eigenstrain must be an array [%d, %d] of tensor components, got shape %s" % (n_cells, ne, e.shape))
    return e


def assemble_anisotropic_load(space, material, eigenstrain, b, add=True):
    """b (+)= int (C : eps*) : grad v dx on a vector CG1 space (fs_assemble_anisotropic_load).  eigenstrain: [n_cells, 6] (xx, yy, zz,
    xy, xz, yz) or [n_cells, 4] (xx, yy, zz, xy) in plane strain, tensor components in global axes, device cell order."""
    keep = []
    nc = space.mesh.info()[1]
    m = _aniso_material(material, nc, keep)
    e = _aniso_eigenstrain(eigenstrain, space, nc)
    if e is None:
        raise BackendError("assemble_anisotropic_load: an eigenstrain is required")
    L.check(L.load().fs_assemble_anisotropic_load(space.h, C.byref(m), L.p_f64(e), b.h, 1 if add else 0), "fs_assemble_anisotropic_load")


def anisotropic_stress(space, u, material, eigenstrain=None, cell_stress=False, p1_space=None, vm_rhs=None):
    """sigma = C : (eps(u) - eps*) per cell on a vector CG1 space (fs_anisotropic_stress); u: DeviceVector of the space's dofs, or None.
    cell_stress=True: returns the array [n_cells, 6] (or [n_cells, 4] in plane strain) in device cell order, else None.  p1_space and
    vm_rhs (both or neither): vm_rhs becomes the right-hand side of the von Mises projection onto the scalar CG1 space."""
    keep = []
    nc = space.mesh.info()[1]
    m = _aniso_material(material, nc, keep)
    e = _aniso_eigenstrain(eigenstrain, space, nc)
    if (p1_space is None) != (vm_rhs is None):
        raise BackendError("anisotropic_stress: p1_space and vm_rhs go together")
    if p1_space is not None:
        _same_device_mesh(space, p1_space, "anisotropic_stress")
    sig = np.empty((nc, 6 if space.ncomp == 3 else 4)) if cell_stress else None
    L.check(L.load().fs_anisotropic_stress(space.h, u.h if u is not None else None, C.byref(m), L.p_f64(e), L.p_f64(sig),
                                           p1_space.h if p1_space is not None else None, vm_rhs.h if vm_rhs is not None else None),
            "fs_anisotropic_stress")
    return sig


HYPER_MODELS = {"neo_hookean": L.FS_HYPER_NEO_HOOKEAN, "st_venant_kirchhoff": L.FS_HYPER_ST_VENANT_KIRCHHOFF,
                "mooney_rivlin": L.FS_HYPER_MOONEY_RIVLIN, "yeoh": L.FS_HYPER_YEOH}
_HYPER_PARAMS = {"mooney_rivlin": 3, "yeoh": 4}           # numbers in the parameter row: (c10, c01, kappa), (c10, c20, c30, kappa)


def _hyper_form(who, space, lame, model, params, add, keep):
    """The fs_hyper_form of a model: neo_hookean / st_venant_kirchhoff read `lame`, mooney_rivlin / yeoh read `params`."""
    if model not in HYPER_MODELS:
        raise BackendError("%s: unknown energy model %r (one of %s)" % (who, model, ", ".join(sorted(HYPER_MODELS))))
    f = L.fs_hyper_form()
    f.model = HYPER_MODELS[model]
    f.add = 1 if add else 0
    nc = space.mesh.info()[1]
    if model in _HYPER_PARAMS:
        n = _HYPER_PARAMS[model]
        if params is None:
            raise BackendError("%s: the %s energy needs params (%d numbers, or ('cell', array[n_cells, %d]))" % (who, model, n, n))
        if _is_cell_lame(params):
            if params[0] != "cell":
                raise BackendError("%s: params are numbers or ('cell', array), got kind %r" % (who, params[0]))
            a = np.asarray(params[1], dtype=np.float64)
            if a.ndim != 2 or a.shape[0] != nc or a.shape[1] not in (n, 4):
                raise BackendError("%s: per-cell %s parameters must be an array [%d, %d], got shape %s" % (who, model, nc, n, a.shape))
            rows = np.zeros((nc, 4))
            rows[:, :n] = a[:, :n]
            keep.append(rows)
            f.cell_params.mode = L.FS_COEF_CELL_HYPER
            f.cell_params.data = L.p_f64(rows)
        else:
            vals = [float(x) for x in params]
            if len(vals) not in (n, 4):
                raise BackendError("%s: the %s energy takes %d parameters, got %d" % (who, model, n, len(vals)))
            for k in range(n):
                f.params[k] = vals[k]
    elif lame is None:
        raise BackendError("%s: the %s energy needs the Lame parameters" % (who, model))
    elif _is_cell_lame(lame):
        f.lame.mode = L.FS_COEF_CELL_LAME
        f.lame.data = L.p_f64(_lame_cells(lame, keep, nc))
    else:
        f.mu, f.lambda_ = float(lame[0]), float(lame[1])
    return f


def assemble_hyperelastic(space, u, lame, K=None, r=None, energy=False, add=False, model='neo_hookean', params=None):
    """Tangent K, internal force r and energy of a hyperelastic material at the displacement u (DeviceVector of the space's dofs) on a
    vector CG1 space (fs_assemble_hyperelastic).  model: 'neo_hookean' (default) or 'st_venant_kirchhoff' with lame = (mu, lambda)
    numbers or ('cell', array[n_cells, 2]); 'mooney_rivlin' with params = (c10, c01, kappa) or 'yeoh' with params = (c10, c20, c30,
    kappa), numbers or ('cell', array[n_cells, 3 or 4]) - lame is not read then.  Per-cell arrays are in device cell order.  K / r:
    the DeviceMatrix / DeviceVector to fill (None: not computed).  Returns {'energy', 'n_inverted', 'first_inverted_cell'}; the
    energy is computed only with energy=True (0.0 otherwise)."""
    keep = []
    f = _hyper_form("assemble_hyperelastic", space, lame, model, params, add, keep)
    what = (L.FS_HYPER_TANGENT if K is not None else 0) | (L.FS_HYPER_FORCE if r is not None else 0) | (L.FS_HYPER_ENERGY if energy else 0)
    info = L.fs_hyper_info()
    L.check(L.load().fs_assemble_hyperelastic(space.h, K.h if K is not None else None, r.h if r is not None else None, u.h,
                                              C.byref(f), int(what), C.byref(info)), "fs_assemble_hyperelastic")
    return {"energy": info.energy if energy else 0.0, "n_inverted": int(info.n_inverted),
            "first_inverted_cell": int(info.first_inverted_cell)}


def hyperelastic_stress(space, u, lame, model='neo_hookean', params=None):
    """Cauchy stress sigma = P F^T / J per cell at the displacement u (fs_hyper_stress), for every model of assemble_hyperelastic with
    the same lame / params: array [n_cells, 6] (xx, yy, zz, xy, xz, yz), in plane strain [n_cells, 4] (xx, yy, zz, xy), device cell
    order.  A state with an inverted cell raises BackendError naming the first one."""
    keep = []
    f = _hyper_form("hyperelastic_stress", space, lame, model, params, False, keep)
    sig = np.empty((space.mesh.info()[1], 6 if space.ncomp == 3 else 4))
    L.check(L.load().fs_hyper_stress(space.h, u.h, C.byref(f), L.p_f64(sig), None), "fs_hyper_stress")
    return sig


class _CellHistory(_Handle):
    """What the per-cell history objects share: the cell and component counts, the map to the caller's cell numbering, and reset /
    commit through the fs_<_prefix>_state_* calls."""
    _prefix = None

    def __init__(self, space, cell_order=None):
        super().__init__()
        self.space = space
        self.n_cells = int(space.mesh.info()[1])
        self.n_comp = 6 if space.ncomp == 3 else 4
        self.cell_order = None if cell_order is None else np.asarray(cell_order, dtype=np.int64)

    def _call(self, name, *args):
        name = "fs_%s_state_%s" % (self._prefix, name)
        L.check(getattr(L.load(), name)(*args), name)

    def reset(self):
        self._call("reset", self.h)

    def commit(self):
        """trial -> committed: the step has converged"""
        self._call("commit", self.h)

    def _to_host(self, a):
        if self.cell_order is None:
            return a
        out = np.empty_like(a)
        out[self.cell_order] = a
        return out


def _cell_material(material, n_cells, width, kind_error, shape_error):
    """The array of a ('cell', array[n_cells, width]) material, None for any other material."""
    if not (isinstance(material, tuple) and len(material) == 2 and isinstance(material[0], str)):
        return None
    if material[0] != "cell":
        raise BackendError(kind_error % (material[0],))
    a = np.ascontiguousarray(material[1], dtype=np.float64)
    if a.shape != (n_cells, width):
        raise BackendError(shape_error % (n_cells, width, a.shape))
    return a


class PlasticHistory(_CellHistory):
    """Per-cell history of the J2 return mapping on a vector CG1 space (fs_plastic_state_*): the committed state (plastic strain,
    cumulative plastic strain, returned stress) and the trial state of the last assemble_plasticity.  The device keeps the cells in
    its own order; ``cell_order`` (device cell -> caller's cell, None: the same order) maps every array that crosses this class, so
    callers see their own cell numbering.  Tensors: (xx, yy, zz, xy, xz, yz) in 3-D, (xx, yy, zz, xy) in plane strain."""
    _destroy = "fs_plastic_state_destroy"
    _prefix = "plastic"

    def __init__(self, space, cell_order=None):
        super().__init__(space, cell_order)
        self._call("create", space.h, C.byref(self.h))

    def get(self, trial=False):
        """(eps_p [n_cells, n_comp], p [n_cells], stress [n_cells, n_comp]) of the committed (or the trial) state"""
        ep, p, sg = np.empty((self.n_cells, self.n_comp)), np.empty(self.n_cells), np.empty((self.n_cells, self.n_comp))
        self._call("get", self.h, L.FS_PLASTIC_TRIAL if trial else L.FS_PLASTIC_COMMITTED, L.p_f64(ep), L.p_f64(p), L.p_f64(sg))
        return self._to_host(ep), self._to_host(p), self._to_host(sg)

    def set(self, eps_p, p):
        """the committed plastic strain and cumulative plastic strain from host arrays in the caller's cell numbering"""
        ep = np.asarray(eps_p, dtype=np.float64).reshape(self.n_cells, self.n_comp)
        p = np.asarray(p, dtype=np.float64).reshape(self.n_cells)
        if self.cell_order is not None:
            ep, p = ep[self.cell_order], p[self.cell_order]
        ep, p = L.f64(ep), L.f64(p)
        self._call("set", self.h, L.p_f64(ep), L.p_f64(p))


def assemble_plasticity(space, u, history, material, K=None, r=None, add=False):
    """Consistent tangent K and internal force r of J2 plasticity at the displacement u (DeviceVector of the space's dofs), from the
    committed state of ``history`` (fs_assemble_plasticity); the trial state is left in ``history``.  material: (mu, lambda,
    yield_stress, hardening) numbers or ('cell', array[n_cells, 4]) in DEVICE cell order.  K / r: the DeviceMatrix / DeviceVector to
    fill (None: not computed).  Returns {'n_yielded', 'n_nonfinite', 'first_nonfinite_cell'}."""
    f = L.fs_plastic_form()
    keep = _cell_material(material, history.n_cells, 4, "plastic material: four numbers or ('cell', array[n_cells, 4]), got kind %r",
                          "per-cell plastic material must be an array [%d, %d], got shape %s")
    if keep is not None:
        f.material.mode = L.FS_COEF_CELL_PLASTIC
        f.material.data = L.p_f64(keep)
    else:
        f.mu, f.lambda_, f.yield_stress, f.hardening = (float(x) for x in material)
    f.add = 1 if add else 0
    what = (L.FS_PLASTIC_TANGENT if K is not None else 0) | (L.FS_PLASTIC_FORCE if r is not None else 0)
    info = L.fs_plastic_info()
    L.check(L.load().fs_assemble_plasticity(space.h, K.h if K is not None else None, r.h if r is not None else None, u.h, history.h,
                                            C.byref(f), int(what), C.byref(info)), "fs_assemble_plasticity")
    return {"n_yielded": int(info.n_yielded), "n_nonfinite": int(info.n_nonfinite), "first_nonfinite_cell": int(info.first_nonfinite_cell)}


class ViscoHistory(_CellHistory):
    """Per-cell history of the Prony-series update on a vector CG1 space (fs_visco_state_*): the committed state (deviatoric strain
    e, viscous strains h_k, stress) and the trial state of the last update.  The device keeps the cells in its own order;
    ``cell_order`` (device cell -> caller's cell, None: the same order) maps every array that crosses this class, so callers see
    their own cell numbering.  Tensors: (xx, yy, zz, xy, xz, yz) in 3-D, (xx, yy, zz, xy) in plane strain."""
    _destroy = "fs_visco_state_destroy"
    _prefix = "visco"

    def __init__(self, space, n_terms, cell_order=None):
        super().__init__(space, cell_order)
        self.n_terms = int(n_terms)
        self._call("create", space.h, self.n_terms, C.byref(self.h))

    def get(self, trial=False):
        """(e [n_cells, n_comp], h [n_cells, n_terms, n_comp], stress [n_cells, n_comp]) of the committed (or the trial) state"""
        e, sg = np.empty((self.n_cells, self.n_comp)), np.empty((self.n_cells, self.n_comp))
        h = np.empty((self.n_cells, self.n_terms, self.n_comp))
        self._call("get", self.h, L.FS_VISCO_TRIAL if trial else L.FS_VISCO_COMMITTED, L.p_f64(e), L.p_f64(h) if self.n_terms else None,
                   L.p_f64(sg))
        return self._to_host(e), self._to_host(h), self._to_host(sg)

    def set(self, e, h):
        """the committed deviatoric strain and viscous strains from host arrays in the caller's cell numbering"""
        e = np.asarray(e, dtype=np.float64).reshape(self.n_cells, self.n_comp)
        h = np.asarray(h, dtype=np.float64).reshape(self.n_cells, self.n_terms, self.n_comp)
        if self.cell_order is not None:
            e, h = e[self.cell_order], h[self.cell_order]
        e, h = L.f64(e), L.f64(h)
        self._call("set", self.h, L.p_f64(e), L.p_f64(h) if self.n_terms else None)


def assemble_viscoelastic(space, history, material, dt, u=None, load=None, force=None, update=None, add=False):
    """The device passes of one viscoelastic step (fs_assemble_viscoelastic).  material: (mu, lambda, [(g_k, tau_k), ...]) with the
    INSTANTANEOUS Lame parameters, or ('cell', array[n_cells, 2 + 2 n_terms]) = (mu, lambda, g_1, tau_1, ...) per cell in DEVICE
    cell order.  load: DeviceVector that receives -int B^T s_hist dx from the committed history; u: displacement (DeviceVector of
    the space's dofs) at which the trial state is updated (update defaults to ``u is not None``); force: DeviceVector that receives
    int B^T sigma dx of the trial stress.  Returns {'n_nonfinite', 'first_nonfinite_cell'} and the device milliseconds of the passes
    that ran ('load_ms', 'update_ms', 'force_ms')."""
    f = L.fs_visco_form()
    nt = history.n_terms
    keep = _cell_material(material, history.n_cells, 2 + 2 * nt, "viscoelastic material: (mu, lambda, terms) or ('cell', array), got kind %r",
                          "per-cell viscoelastic material must be an array [%d, %d], got shape %s")
    if keep is not None:
        f.material.mode = L.FS_COEF_CELL_VISCO
        f.material.data = L.p_f64(keep)
        f.n_terms = nt
    else:
        mu, lmbda, terms = material
        terms = [(float(g), float(tau)) for g, tau in terms]
        if len(terms) > L.FS_VISCO_MAX_TERMS:
            raise BackendError("viscoelastic material: %d Prony terms, at most %d are supported" % (len(terms), L.FS_VISCO_MAX_TERMS))
        f.mu, f.lambda_, f.n_terms = float(mu), float(lmbda), len(terms)
        for k, (g, tau) in enumerate(terms):
            f.g[k], f.tau[k] = g, tau
    f.dt = float(dt)
    f.add = 1 if add else 0
    if load is not None and force is not None:
        raise BackendError("assemble_viscoelastic: the history load and the internal force are separate calls")
    if update is None:
        update = u is not None
    what = (L.FS_VISCO_LOAD if load is not None else 0) | (L.FS_VISCO_UPDATE if update else 0) | (L.FS_VISCO_FORCE if force is not None else 0)
    r = load if load is not None else force
    info = L.fs_visco_info()
    L.check(L.load().fs_assemble_viscoelastic(space.h, r.h if r is not None else None, u.h if u is not None else None, history.h,
                                              C.byref(f), int(what), C.byref(info)), "fs_assemble_viscoelastic")
    return {"n_nonfinite": int(info.n_nonfinite), "first_nonfinite_cell": int(info.first_nonfinite_cell), "load_ms": info.load_ms,
            "update_ms": info.update_ms, "force_ms": info.force_ms}


class _MarcherState(_Handle):
    """What the device states of the time marchers share: creation on a space, the size check of a host field, the Dirichlet
    arguments of configure() and the batch call of the two explicit marchers.  Arrays are in DEVICE dof order."""
    _create = None

    def __init__(self, space):
        super().__init__()
        self.space = space
        self.n = int(space.n_owned)
        L.check(getattr(L.load(), self._create)(space.h, C.byref(self.h)), self._create)

    def _field(self, a, who, name):
        a = L.f64(a).ravel()
        if a.size != self.n:
            raise BackendError("%s.%s: %s has %d entries, the space has %d dofs" % (type(self).__name__, who, name, a.size, self.n))
        return a

    @staticmethod
    def _dirichlet(dofs, values):
        """the Dirichlet dofs and values of a configure() call as the arrays the library takes; a scalar value serves every dof"""
        dofs = L.i32([] if dofs is None else dofs).ravel()
        return dofs, L.f64(np.broadcast_to(0.0 if values is None else values, dofs.shape))

    def _batch_advance(self, entry, head, load_scale, dirichlet_scale, receivers, traces, energy, info):
        """len(load_scale) steps on the device without a host round trip through the entry point `entry`, whose leading arguments
        (the matrix and the state, or the state and its material) are `head`; step k of the call
        advances n -> n+1 with load_scale[k] = s_f[n] and dirichlet_scale[k] = s_g[n+1].  Returns {'traces': [n_steps, n_receivers]
        or None, 'energy': [n_steps, 2] = (kinetic, potential) or None, and with info 'device_ms', 'n_nonfinite',
        'first_nonfinite_step', 'step'}."""
        sf, sg = L.f64(load_scale).ravel(), L.f64(dirichlet_scale).ravel()
        if sf.size != sg.size:
            raise BackendError("%s.advance: %d load factors and %d Dirichlet factors" % (type(self).__name__, sf.size, sg.size))
        ns = sf.size
        rec = L.i32([] if receivers is None else receivers).ravel()
        tr = np.empty((ns, rec.size)) if (traces and rec.size) else None
        en = np.empty((ns, 2)) if energy else None
        inf = L.fs_march_info() if info else None
        L.check(getattr(L.load(), entry)(*head, ns, L.p_f64(sf), L.p_f64(sg), rec.size, L.p_i32(rec) if rec.size else None,
                                         L.p_f64(tr), L.p_f64(en), C.byref(inf) if info else None), entry)
        out = {"traces": tr, "energy": en}
        if info:
            out.update(device_ms=inf.device_ms, n_nonfinite=int(inf.n_nonfinite), first_nonfinite_step=int(inf.first_nonfinite_step),
                       step=int(inf.step))
        return out


class WaveState(_MarcherState):
    """Device state of the explicit wave marcher on a scalar CG1 space (fs_wave_state_*): u^{n-1}, u^n and a work field, the lumped
    mass m, the lumped boundary damping d, the load F, the Dirichlet dofs with their values, and the step counter n.  Arrays are in
    DEVICE dof order."""
    _create, _destroy = "fs_wave_state_create", "fs_wave_state_destroy"

    def configure(self, dt, mass, damping=None, load=None, dirichlet_dofs=None, dirichlet_values=None):
        m, d, f = (None if a is None else self._field(a, "configure", name) for a, name in ((mass, "mass"), (damping, "damping"), (load, "load")))
        dofs, vals = self._dirichlet(dirichlet_dofs, dirichlet_values)
        L.check(L.load().fs_wave_state_configure(self.h, float(dt), L.p_f64(m), L.p_f64(d), L.p_f64(f), dofs.size, L.p_i32(dofs),
                                                 L.p_f64(vals)), "fs_wave_state_configure")

    def set(self, u_prev, u, step):
        a, b = self._field(u_prev, "set", "u_prev"), self._field(u, "set", "u")
        L.check(L.load().fs_wave_state_set(self.h, L.p_f64(a), L.p_f64(b), int(step)), "fs_wave_state_set")

    def get(self):
        """(u^{n-1}, u^n, n)"""
        a, b, k = np.empty(self.n), np.empty(self.n), C.c_int64(0)
        L.check(L.load().fs_wave_state_get(self.h, L.p_f64(a), L.p_f64(b), C.byref(k)), "fs_wave_state_get")
        return a, b, k.value

    def start(self, K, u0, v0, load_scale0=1.0, dirichlet_scale1=1.0):
        """u^1 from (u^0, v^0): the state then holds (u^0, u^1), n = 1"""
        a, b = self._field(u0, "start", "u0"), self._field(v0, "start", "v0")
        L.check(L.load().fs_wave_start(K.h, self.h, L.p_f64(a), L.p_f64(b), float(load_scale0), float(dirichlet_scale1)), "fs_wave_start")

    def advance(self, K, load_scale, dirichlet_scale, receivers=None, traces=True, energy=True, info=True):
        """a batch of steps through fs_wave_advance: see _MarcherState._batch_advance"""
        return self._batch_advance("fs_wave_advance", (K.h, self.h), load_scale, dirichlet_scale, receivers, traces, energy, info)


def wave_advance(K, state, load_scale, dirichlet_scale, receivers=None, traces=True, energy=True, info=True):
    """A batch of explicit wave steps with the stiffness K on a WaveState (fs_wave_advance): see WaveState.advance."""
    return state.advance(K, load_scale, dirichlet_scale, receivers=receivers, traces=traces, energy=energy, info=info)


class DynamicsState(_MarcherState):
    """Device state of the generalized-alpha marcher on a vector CG1 / CG2 space (fs_dyn_*): u, v, a, the work vectors p, q, M p,
    K q, the load F, the Dirichlet dofs with their values, the constants of the scheme and the step counter n.  Arrays are in DEVICE
    dof order.  K and M are the operators WITHOUT eliminated rows; the solve between predict() and correct() is the caller's."""
    _create, _destroy = "fs_dyn_state_create", "fs_dyn_state_destroy"

    def configure(self, dt, alpha_m, alpha_f, beta, gamma, eta_m=0.0, eta_k=0.0, load=None, dirichlet_dofs=None, dirichlet_values=None):
        f = None if load is None else self._field(load, "configure", "load")
        dofs, vals = self._dirichlet(dirichlet_dofs, dirichlet_values)
        L.check(L.load().fs_dyn_state_configure(self.h, float(dt), float(alpha_m), float(alpha_f), float(beta), float(gamma), float(eta_m),
                                                float(eta_k), L.p_f64(f), dofs.size, L.p_i32(dofs), L.p_f64(vals)), "fs_dyn_state_configure")

    def set(self, u, v, a, step=0):
        u, v, a = (self._field(x, "set", nm) for x, nm in ((u, "u"), (v, "v"), (a, "a")))
        L.check(L.load().fs_dyn_state_set(self.h, L.p_f64(u), L.p_f64(v), L.p_f64(a), int(step)), "fs_dyn_state_set")

    def get(self):
        """(u, v, a, n)"""
        u, v, a, k = np.empty(self.n), np.empty(self.n), np.empty(self.n), C.c_int64(0)
        L.check(L.load().fs_dyn_state_get(self.h, L.p_f64(u), L.p_f64(v), L.p_f64(a), C.byref(k)), "fs_dyn_state_get")
        return u, v, a, k.value

    def work(self):
        """(p, q, M p, K q) of the last predict()"""
        out = [np.empty(self.n) for _ in range(4)]
        L.check(L.load().fs_dyn_state_get_work(self.h, *[L.p_f64(x) for x in out]), "fs_dyn_state_get_work")
        return tuple(out)

    def info(self):
        """waits for the device: {'predict_ms', 'predict_pointwise_ms', 'correct_ms', 'n_nonfinite', 'first_nonfinite_step', 'step'}"""
        inf = L.fs_dyn_info()
        L.check(L.load().fs_dyn_state_info(self.h, C.byref(inf)), "fs_dyn_state_info")
        return {k: getattr(inf, k) for k, _ in L.fs_dyn_info._fields_}

    def start_rhs(self, K, M, u0, v0, load_scale0, rhs):
        """takes (u_0, v_0); rhs (a DeviceVector) = s_f(t_0) F - C v_0 - K u_0 on the free rows, 0 on the Dirichlet rows"""
        u0, v0 = self._field(u0, "start_rhs", "u0"), self._field(v0, "start_rhs", "v0")
        L.check(L.load().fs_dyn_start_rhs(K.h, M.h, self.h, L.p_f64(u0), L.p_f64(v0), float(load_scale0), rhs.h), "fs_dyn_start_rhs")

    def start(self, a0):
        """a_0 (a DeviceVector, solved from start_rhs with the eliminated M): the state then holds (u_0, v_0, a_0), n = 0"""
        L.check(L.load().fs_dyn_start(self.h, a0.h), "fs_dyn_start")

    def predict(self, K, M, load_scale, dirichlet_scale_next, rhs):
        """rhs (a DeviceVector) of the step n -> n+1; nothing returns to the host"""
        L.check(L.load().fs_dyn_predict(K.h, M.h, self.h, float(load_scale), float(dirichlet_scale_next), rhs.h), "fs_dyn_predict")

    def correct(self, x, receivers=None):
        """x (a DeviceVector) = u_{n+1}: forms a_{n+1}, v_{n+1}; with receivers returns the samples of u_{n+1} at those dofs (and
        waits for the device), else None"""
        rec = L.i32([] if receivers is None else receivers).ravel()
        out = np.empty(rec.size) if rec.size else None
        L.check(L.load().fs_dyn_correct(self.h, x.h, rec.size, L.p_i32(rec) if rec.size else None, L.p_f64(out)), "fs_dyn_correct")
        return out

    def energy(self, K, M):
        """(1/2 v^T M v, 1/2 u^T K u)"""
        out = np.empty(2)
        L.check(L.load().fs_dyn_energy(K.h, M.h, self.h, L.p_f64(out)), "fs_dyn_energy")
        return float(out[0]), float(out[1])


class _LeapfrogState(_MarcherState):
    """What the device states of the two central-difference ("leapfrog") marchers share: every call but the ones that are a
    marcher's own.  _api is the prefix of the entry points, _head(K) their leading arguments: the matrix and the state, or the
    state and its material.  The state is (u_n, w_n = v_{n-1/2}, n)."""
    _api = None

    def _call(self, name, *args):
        entry = "%s_%s" % (self._api, name)
        L.check(getattr(L.load(), entry)(*args), entry)

    def configure(self, dt, eta_m, mass, load=None, dirichlet_dofs=None, dirichlet_values=None):
        m = self._field(mass, "configure", "mass")
        f = None if load is None else self._field(load, "configure", "load")
        dofs, vals = self._dirichlet(dirichlet_dofs, dirichlet_values)
        self._call("state_configure", self.h, float(dt), float(eta_m), L.p_f64(m), L.p_f64(f), dofs.size, L.p_i32(dofs), L.p_f64(vals))

    def set(self, u, w, step):
        u, w = self._field(u, "set", "u"), self._field(w, "set", "w")
        self._call("state_set", self.h, L.p_f64(u), L.p_f64(w), int(step))

    def get(self):
        """(u_n, w_n = v_{n-1/2}, n)"""
        u, w, k = np.empty(self.n), np.empty(self.n), C.c_int64(0)
        self._call("state_get", self.h, L.p_f64(u), L.p_f64(w), C.byref(k))
        return u, w, k.value

    def _start(self, K, u0, v0, load_scale0, dirichlet_scale0, dirichlet_scale1):
        u0, v0 = self._field(u0, "start", "u0"), self._field(v0, "start", "v0")
        self._call("start", *self._head(K), L.p_f64(u0), L.p_f64(v0), float(load_scale0), float(dirichlet_scale0), float(dirichlet_scale1))

    def _advance(self, K, load_scale, dirichlet_scale, receivers, traces, energy, info):
        return self._batch_advance(self._api + "_advance", self._head(K), load_scale, dirichlet_scale, receivers, traces, energy, info)

    def _full_step(self, K, load_scale_n):
        v, a = np.empty(self.n), np.empty(self.n)
        self._call("full_step", *self._head(K), float(load_scale_n), L.p_f64(v), L.p_f64(a))
        return v, a


class ExplicitDynamicsState(_LeapfrogState):
    """Device state of the central-difference marcher on a vector CG1 space (fs_dyn_explicit_*): u_n, w_n = v_{n-1/2}, the last
    product y = K u, the lumped mass m, the load F, the Dirichlet dofs with their values, dt, eta_M and the step counter n.  Arrays
    are in DEVICE dof order.  K is the operator WITHOUT eliminated rows."""
    _create, _destroy, _api = "fs_dyn_explicit_state_create", "fs_dyn_explicit_state_destroy", "fs_dyn_explicit"

    def _head(self, K):
        return K.h, self.h

    def work(self):
        """y = K u of the last product"""
        y = np.empty(self.n)
        self._call("state_get_work", self.h, L.p_f64(y))
        return y

    def start(self, K, u0, v0, load_scale0=1.0, dirichlet_scale0=1.0, dirichlet_scale1=1.0):
        """(u_1, w_{1/2}) from (u_0, v_0): n = 1"""
        self._start(K, u0, v0, load_scale0, dirichlet_scale0, dirichlet_scale1)

    def advance(self, K, load_scale, dirichlet_scale, receivers=None, traces=True, energy=True, info=True):
        """a batch of steps through fs_dyn_explicit_advance: see _MarcherState._batch_advance"""
        return self._advance(K, load_scale, dirichlet_scale, receivers, traces, energy, info)

    def full_step(self, K, load_scale_n):
        """(v_n, a_n) of the state's time point under s_f[n] = load_scale_n: one product, the state does not change"""
        return self._full_step(K, load_scale_n)


class HyperelasticDynamicsState(_LeapfrogState):
    """Device state of the explicit finite-strain marcher on a vector CG1 space (fs_hyper_dyn_*): u_n (double-buffered inside the
    library), w_n = v_{n-1/2}, the lumped mass m, the load F, the Dirichlet dofs with their values, dt, eta_M, the step counter n
    and the device copy of the material.  Arrays are in DEVICE dof order.  The material is given once, as for
    assemble_hyperelastic (per-cell arrays in device cell order); there is no matrix: every step evaluates the internal force."""
    _create, _destroy, _api = "fs_hyper_dyn_state_create", "fs_hyper_dyn_state_destroy", "fs_hyper_dyn"

    def __init__(self, space, lame=None, model='neo_hookean', params=None):
        super().__init__(space)
        self._keep = []
        self._form = _hyper_form("HyperelasticDynamicsState", space, lame, model, params, False, self._keep)

    def _head(self, K=None):
        return self.h, C.byref(self._form)

    def start(self, u0, v0, load_scale0=1.0, dirichlet_scale0=1.0, dirichlet_scale1=1.0):
        """(u_1, w_{1/2}) from (u_0, v_0): n = 1"""
        self._start(None, u0, v0, load_scale0, dirichlet_scale0, dirichlet_scale1)

    def advance(self, load_scale, dirichlet_scale, receivers=None, traces=True, energy=True, info=True):
        """a batch of steps through fs_hyper_dyn_advance: see _MarcherState._batch_advance; energy[k] = (E_kin(w_{n+1/2}), Pi(u_n))"""
        return self._advance(None, load_scale, dirichlet_scale, receivers, traces, energy, info)

    def full_step(self, load_scale_n):
        """(v_n, a_n) of the state's time point under s_f[n] = load_scale_n: the force is recomputed, the state does not change"""
        return self._full_step(None, load_scale_n)

    def internal_force(self):
        """(f_int(u_n), Pi(u_n)) of the held state"""
        f, e = np.empty(self.n), C.c_double(0.0)
        self._call("internal_force", *self._head(), L.p_f64(f), C.byref(e))
        return f, e.value


def assemble_viscous_stress(th_space, w, nu, p1_space, b, viscosity_law=None):
    """b[vertex*9 + 3i + j] = int (nu (grad u + grad u^T) - p I)_ij phi_vertex dx for a Taylor-Hood iterate w.
    viscosity_law = (p_ref, exponent): nu (p / p_ref)^exponent."""
    pref, ex = (0.0, 0.0) if viscosity_law is None else (float(viscosity_law[0]), float(viscosity_law[1]))
    _same_device_mesh(th_space, p1_space, "assemble_viscous_stress")
    L.check(L.load().fs_assemble_viscous_stress_nn(th_space.h, w.h, float(nu), p1_space.h, b.h, pref, ex), "fs_assemble_viscous_stress")


def set_dirichlet_values(b, dofs, vals):
    dofs = L.i32(dofs).ravel()
    vals = L.f64(np.broadcast_to(vals, dofs.shape))
    L.check(L.load().fs_apply_dirichlet(None, b.h, dofs.size, L.p_i32(dofs), L.p_f64(vals), 0), "fs_apply_dirichlet")


def krylov_solve(A, b, x, rtol=1e-8, atol=0.0, max_iter=10000, precond="jacobi", batch=0, nonzero_guess=False,
                 method="cg", diagonal_scale=True, norm="unpreconditioned", pipelined=None):
    """CG (SPD) or BiCGStab (non-symmetric) on the device.  Returns a stats dict.
    pipelined: True selects the Ghysels-Vanroose recurrence (the all-reduce of the sums hidden under the product, 112 instead
    of 72 B/DOF of vector traffic); None / False (default) the single-reduction recurrence - in every measurement so far the
    pipelined one was slower, so it is opt-in."""
    o = L.fs_krylov_opts()
    o.method = {"cg": L.FS_KSP_CG, "bicgstab": L.FS_KSP_BICGSTAB}[method]
    o.precond = {"none": L.FS_PC_NONE, None: L.FS_PC_NONE, "jacobi": L.FS_PC_JACOBI}[precond]
    o.rtol, o.atol, o.max_iter, o.batch = float(rtol), float(atol), int(max_iter), int(batch)
    o.nonzero_guess = 1 if nonzero_guess else 0
    o.diagonal_scale = 1 if diagonal_scale else 0
    o.pipelined = -1 if pipelined is None else (1 if pipelined else 0)
    if o.pipelined < 0 and not (method == "cg" and o.precond == L.FS_PC_JACOBI and diagonal_scale):
        o.pipelined = 0
    o.norm_type = {"unpreconditioned": L.FS_NORM_UNPRECONDITIONED, "preconditioned": L.FS_NORM_PRECONDITIONED}[norm]
    st = L.fs_krylov_stats()

    def solve():
        L.check(L.load().fs_krylov_solve(A.h, b.h, x.h, C.byref(o), C.byref(st)), "fs_krylov_solve")
    _with_p2p_fallback(A.space, solve, x if nonzero_guess else None)
    return {k: getattr(st, k) for k, _ in L.fs_krylov_stats._fields_}


def _with_p2p_fallback(spaces, solve, x_guess=None):
    """Run a solve over space(s) whose ghost refresh is the peer-to-peer exchange.  A wait of that transport that times out (peer
    process gone, stores over the mappings not visible on this system) fails the solve with FS_ERR_P2P_TIMEOUT on the rank that
    saw it.  The ranks then compare notes over RCCL proper (never over the transport in doubt) on THAT code only, and if any of
    them saw it ALL of them turn the exchange of the space(s) off and solve again over RCCL send / recv - also a rank whose own
    solve failed with another code (stale ghosts produce a breakdown as easily as a time-out; a rank that raised here would leave
    the others alone in the collectives of the second solve).  When NO rank timed out, any failure - a Krylov breakdown, a zero
    diagonal, a bad argument - is not the transport's: it is raised as it is (after the agreement, so that the ranks stay
    paired), nothing is turned off and nothing is repeated.  One small RCCL all-gather per solve, only while the
    exchange is on: a rank can finish its last wait while a neighbour times out on its own, so success on this rank says nothing
    about the others."""
    if not isinstance(spaces, (list, tuple)):
        spaces = [spaces]
    live = []
    for sp in spaces:
        if sp is not None and getattr(sp, "_p2p", False) and not any(sp is q for q in live):
            live.append(sp)
    if not live or not _comm_up:
        return solve()
    keep = None
    if x_guess is not None:
        keep = DeviceVector(x_guess.n)
        keep.copy_from(x_guess)
    err = None
    try:
        solve()
    except L.BackendError as e:
        err = e
    timed_out = err is not None and err.rc == L.FS_ERR_P2P_TIMEOUT
    if float(np.sum(comm_allgather([1.0 if timed_out else 0.0], 1))) == 0.0:
        if err is not None:
            raise err
        return None
    import logging
    logging.getLogger("fenicssolver_amd").warning("peer-to-peer halo exchange timed out during a solve (%s): turned off, solving again over RCCL",
                                                  "on this rank" if timed_out else "on another rank")
    for sp in live:
        sp.enable_p2p_halo(False)
    # Once ANY rank timed out, every local error of this solve is taken as a consequence of it (a rank whose neighbour's stores never
    # arrived consumes stale ghosts or garbage sums and may fail with a breakdown instead of the time-out code): ALL ranks solve
    # again over RCCL, so that nobody is left alone in a collective.  A genuine non-transport failure shows again in the
    # second solve, on every rank alike, and is raised there.
    if err is not None and not timed_out:
        logging.getLogger("fenicssolver_amd").warning("this rank's solve failed with %r while another rank's exchange timed out: "
                                                      "treated as a consequence, solving again", err)
    if keep is not None:
        x_guess.copy_from(keep)
    return solve()


class AMG(_Handle):
    """Smoothed-aggregation hierarchy of an assembled SPD matrix (PETSc GAMG behind
    PETScPreconditioner("petsc_amg"), SolverBase.py:643-672).  nullspace: [nb, n_dofs] near-null-space
    vectors, "rigid_body" = the six rigid-body modes built on the device from the node coordinates (3-vector CG1
    / CG2 spaces: vertices and edge mid-points), or None = constants per component."""
    _destroy = "fs_amg_destroy"

    def __init__(self, A, nullspace=None, strength_threshold=0.0, max_levels=0, coarse_size=0, smoother_steps=0,
                 eig_steps=0):
        super().__init__()
        self.A = A                      # keeps the matrix alive
        o = L.fs_amg_opts()
        o.strength_threshold, o.max_levels, o.coarse_size = float(strength_threshold), int(max_levels), int(coarse_size)
        o.smoother_steps, o.eig_steps = int(smoother_steps), int(eig_steps)
        ns, nb = None, 0
        if isinstance(nullspace, str):
            if nullspace != "rigid_body":
                raise ValueError("nullspace must be an array, None or 'rigid_body'")
            o.rigid_body_modes = 1
        elif nullspace is not None:
            ns = np.ascontiguousarray(np.asarray(nullspace, dtype=np.float64).reshape(len(nullspace), -1))
            nb = ns.shape[0]
            if ns.shape[1] != A.space.n_owned:
                raise ValueError("near-null space has %d entries per vector, the matrix has %d rows" % (ns.shape[1], A.space.n_owned))
        L.check(L.load().fs_amg_setup(A.h, nb, L.p_f64(ns), C.byref(o), C.byref(self.h)), "fs_amg_setup")

    def attach_distributed_fine(self, A_local, owned_global_nodes):
        """The hierarchy was built on the undecomposed operator: from now on level 0 works on A_local, this rank's rows of the
        decomposed operator (owned_global_nodes[i] = undecomposed node of local owned node i); levels >= 1 stay replicated."""
        g = L.i32(owned_global_nodes)
        L.check(L.load().fs_amg_attach_distributed_fine(self.h, A_local.h, len(g), L.p_i32(g)), "fs_amg_attach_distributed_fine")
        self.A_local = A_local          # keeps the decomposed operator alive

    def info(self):
        nl, oc, gc, ms = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        L.check(L.load().fs_amg_info(self.h, C.byref(nl), C.byref(oc), C.byref(gc), C.byref(ms)), "fs_amg_info")
        return {"levels": nl.value, "operator_complexity": oc.value, "grid_complexity": gc.value, "setup_ms": ms.value}

    def level_info(self, level):
        nn, pn, bs, pc, nz, lm = C.c_int64(), C.c_int64(), C.c_int(), C.c_int(), C.c_int64(), C.c_double()
        L.check(L.load().fs_amg_level_info(self.h, int(level), C.byref(nn), C.byref(bs), C.byref(nz), C.byref(pn),
                                           C.byref(pc), C.byref(lm)), "fs_amg_level_info")
        return {"n_nodes": nn.value, "block_size": bs.value, "nnz_blocks": nz.value, "p_nnz_blocks": pn.value,
                "p_block_cols": pc.value, "lambda_max": lm.value}

    def level_aggregates(self, level):
        """The aggregate (node of level+1) of every node of a level with a prolongator, int32, -1 = in none."""
        out = np.empty(self.level_info(level)["n_nodes"], dtype=np.int32)
        L.check(L.load().fs_amg_level_get(self.h, int(level), 4, None, L.p_i32(out), None), "fs_amg_level_get")
        return out

    def level_blocks(self, level, which="A"):
        """The raw block CSR of a level operator ('A') or of the prolongator from level+1 ('P'): (rowptr, col, val[nnz, br, bc]),
        the structural blocks in the library's order, zeros included."""
        li = self.level_info(level)
        nnz, bc = (li["nnz_blocks"], li["block_size"]) if which == "A" else (li["p_nnz_blocks"], li["p_block_cols"])
        rp = np.empty(li["n_nodes"] + 1, dtype=np.int32)
        ci = np.empty(nnz, dtype=np.int32)
        va = np.empty(nnz * li["block_size"] * bc)
        L.check(L.load().fs_amg_level_get(self.h, int(level), 0 if which == "A" else 1, L.p_i32(rp), L.p_i32(ci),
                                          L.p_f64(va)), "fs_amg_level_get")
        return rp, ci, va.reshape(nnz, li["block_size"], bc)

    def level_matrix(self, level, which="A"):
        """scipy BSR copy of a level operator ('A') or of the prolongator from level+1 ('P')."""
        import scipy.sparse as sp
        li = self.level_info(level)
        if which == "A":
            nnz, br, bc, nrows = li["nnz_blocks"], li["block_size"], li["block_size"], li["n_nodes"]
            ncols = nrows
        else:
            nnz, br, bc, nrows = li["p_nnz_blocks"], li["block_size"], li["p_block_cols"], li["n_nodes"]
            ncols = self.level_info(level + 1)["n_nodes"]
        rp = np.empty(nrows + 1, dtype=np.int32)
        ci = np.empty(nnz, dtype=np.int32)
        va = np.empty(nnz * br * bc)
        L.check(L.load().fs_amg_level_get(self.h, int(level), 0 if which == "A" else 1, L.p_i32(rp), L.p_i32(ci),
                                          L.p_f64(va)), "fs_amg_level_get")
        return sp.bsr_matrix((va.reshape(nnz, br, bc), ci, rp), shape=(nrows * br, ncols * bc)).tocsr()

    def level_nullspace(self, level, nb):
        li = self.level_info(level)
        out = np.empty(li["n_nodes"] * li["block_size"] * nb)
        L.check(L.load().fs_amg_level_get(self.h, int(level), 2, None, None, L.p_f64(out)), "fs_amg_level_get")
        return out.reshape(-1, nb)

    def coarse_inverse(self):
        """The dense inverse that the V-cycle applies on the coarsest level ([n, n], row-major), or None where it runs Chebyshev
        sweeps there instead (a single level, or a coarsest level of more than 2500 rows)."""
        last = self.info()["levels"] - 1
        li = self.level_info(last)
        n = li["n_nodes"] * li["block_size"]
        rc = L.load().fs_amg_level_get(self.h, last, 3, None, None, None)        # no buffer: only asks whether there is one
        if rc == L.FS_ERR_UNSUPPORTED:
            return None
        L.check(rc, "fs_amg_level_get")
        out = np.empty(n * n)
        L.check(L.load().fs_amg_level_get(self.h, last, 3, None, None, L.p_f64(out)), "fs_amg_level_get")
        return out.reshape(n, n)

    def apply(self, r, z):
        L.check(L.load().fs_amg_apply(self.h, r.h, z.h), "fs_amg_apply")

    def solve(self, b, x, rtol=1e-8, atol=0.0, max_iter=500, nonzero_guess=False, norm="unpreconditioned"):
        o = L.fs_krylov_opts()
        o.rtol, o.atol, o.max_iter = float(rtol), float(atol), int(max_iter)
        o.nonzero_guess = 1 if nonzero_guess else 0
        o.norm_type = {"unpreconditioned": L.FS_NORM_UNPRECONDITIONED, "preconditioned": L.FS_NORM_PRECONDITIONED}[norm]
        st = L.fs_krylov_stats()

        def solve():
            L.check(L.load().fs_amg_solve(self.h, b.h, x.h, C.byref(o), C.byref(st)), "fs_amg_solve")
        fine = getattr(self, "A_local", None) or self.A
        _with_p2p_fallback(fine.space, solve, x if nonzero_guess else None)
        return {k: getattr(st, k) for k, _ in L.fs_krylov_stats._fields_}


def _handles(vectors):
    arr = (C.c_void_p * len(vectors))()
    for i, v in enumerate(vectors):
        arr[i] = v.h.value
    return arr


def spmv_multi(A, X, Y):
    """Y[j] = A X[j] for every column in one pass over A's values per chunk of columns (vector spaces of 2 or 3 components);
    each Y[j] equals A.spmv(X[j], Y[j]) bit for bit."""
    if len(X) != len(Y) or not X:
        raise ValueError("spmv_multi: X and Y must be non-empty lists of one length")
    L.check(L.load().fs_spmv_multi(A.h, len(X), _handles(X), _handles(Y)), "fs_spmv_multi")


def gram(X, Y):
    """G[i, j] = X[i] . Y[j] on the device (deterministic)."""
    G = np.empty((len(X), len(Y)))
    L.check(L.load().fs_vector_gram(len(X), _handles(X), len(Y), _handles(Y), L.p_f64(G)), "fs_vector_gram")
    return G


def eigen_solve(K, M, n_modes, amg=None, constrained=None, tol=1e-8, max_iter=500, shift=0.0, block=0, seed=2024):
    """The n_modes smallest eigenpairs of K phi = lambda M phi on the dofs outside `constrained` (LOBPCG on the device, preconditioned
    by one V-cycle of `amg` per column or by Jacobi).  K holds K + shift M when shift > 0; the eigenvalues returned are lambda.
    Returns (eigenvalues [n_modes], modes [DeviceVector, M-orthonormal], stats dict)."""
    o = L.fs_eigen_opts()
    o.n_modes, o.block, o.tol, o.max_iter, o.shift, o.seed = int(n_modes), int(block), float(tol), int(max_iter), float(shift), int(seed)
    cons = L.i32(np.zeros(0) if constrained is None else constrained).ravel()
    modes = [DeviceVector(K.space.n_owned) for _ in range(int(n_modes))]
    lam = np.empty(int(n_modes))
    st = L.fs_eigen_stats()
    L.check(L.load().fs_eigen_solve(K.h, M.h, amg.h if amg is not None else None, cons.size, L.p_i32(cons) if cons.size else None,
                                    C.byref(o), L.p_f64(lam), _handles(modes), C.byref(st)), "fs_eigen_solve")
    return lam, modes, {k: getattr(st, k) for k, _ in L.fs_eigen_stats._fields_}


def spmv_multi_pencil(K, KG, X, YK, YG):
    """YK[j] = K X[j] and YG[j] = KG X[j] for every column in one pass over the pattern per chunk of columns (fs_spmv_multi_pencil):
    KG, whose node-pair blocks must be s I (DeviceMatrix.assemble_geometric), is read from a copy of one double per block.  YK[j]
    equals spmv_multi(K) bit for bit, YG[j] equals spmv_multi(KG) as numbers."""
    if not X or len(X) != len(YK) or len(X) != len(YG):
        raise ValueError("spmv_multi_pencil: X, YK and YG must be non-empty lists of one length")
    L.check(L.load().fs_spmv_multi_pencil(K.h, KG.h, len(X), _handles(X), _handles(YK), _handles(YG)), "fs_spmv_multi_pencil")


def spmv_multi_pencil_benchmark(K, KG, m=8, reps=20):
    """(fused_ms, two_pass_ms): the mean time of one fused pencil product of m columns and of the two block products it replaces
    (HIP events after a warm-up, kernels only)."""
    a, b = C.c_double(0.0), C.c_double(0.0)
    L.check(L.load().fs_spmv_multi_pencil_benchmark(K.h, KG.h, int(m), int(reps), C.byref(a), C.byref(b)), "fs_spmv_multi_pencil_benchmark")
    return a.value, b.value


def buckling_solve(K, KG, n_modes, amg=None, constrained=None, tol=1e-8, max_iter=500, block=0, seed=2024, two_pass=False):
    """The n_modes smallest positive factors lambda of (K + lambda KG) phi = 0 on the dofs outside `constrained` (fs_buckling_solve:
    the LOBPCG of eigen_solve on KG phi = nu K phi, preconditioned by one V-cycle of `amg` - a hierarchy of K - per column, or by the
    Jacobi diagonal of K).  KG as assemble_geometric leaves it, without Dirichlet rows.  two_pass=True: K S and KG S by two block
    products instead of the fused pencil product.  Returns (factors [n_modes] ascending, modes [DeviceVector, K-orthonormal], stats
    dict); a load with fewer than n_modes buckling modes raises BackendError (rc FS_ERR_NUMERIC, "only N buckling mode(s)")."""
    o = L.fs_buckling_opts()
    o.n_modes, o.block, o.tol, o.max_iter, o.seed, o.two_pass = int(n_modes), int(block), float(tol), int(max_iter), int(seed), int(bool(two_pass))
    cons = L.i32(np.zeros(0) if constrained is None else constrained).ravel()
    modes = [DeviceVector(K.space.n_owned) for _ in range(int(n_modes))]
    lam = np.empty(int(n_modes))
    st = L.fs_buckling_stats()
    L.check(L.load().fs_buckling_solve(K.h, KG.h, amg.h if amg is not None else None, cons.size, L.p_i32(cons) if cons.size else None,
                                       C.byref(o), L.p_f64(lam), _handles(modes), C.byref(st)), "fs_buckling_solve")
    return lam, modes, {k: getattr(st, k) for k, _ in L.fs_buckling_stats._fields_}


def assemble_navier_stokes(J, g, w0, w_prev=None, nu=1.0, rho=1.0, inv_dt=0.0, body_force=(0.0, 0.0, 0.0),
                           convection=True, newton=True, mesh_velocity=(0.0, 0.0, 0.0), g2=None, viscosity_law=None):
    """Linearised Taylor-Hood system at the state w0 (J w_new = g), J on a DeviceSpace(mesh, ncomp=4, degree=2).
    g2 = (mode, kappa1): the G2 streamline term (mode 1: Re <= 1, 2: convection dominated).
    viscosity_law = (p_ref, exponent): nu (p0 / p_ref)^exponent with the pressure of w0 (the reference's non-Newtonian law)."""
    f = L.fs_ns_form()
    f.kinematic_viscosity, f.density, f.inv_dt = float(nu), float(rho), float(inv_dt)
    for i in range(3):
        f.body_force[i] = float(body_force[i])
        f.mesh_velocity[i] = float(mesh_velocity[i])
    f.convection, f.newton = (1 if convection else 0), (1 if newton else 0)
    if g2 is not None:
        f.g2_mode, f.g2_kappa1 = int(g2[0]), float(g2[1])
    if viscosity_law is not None:
        f.viscosity_pressure_ref, f.viscosity_pressure_exponent = float(viscosity_law[0]), float(viscosity_law[1])
    L.check(L.load().fs_assemble_navier_stokes(J.h, g.h, w0.h if w0 is not None else None,
                                               w_prev.h if w_prev is not None else None, C.byref(f)),
            "fs_assemble_navier_stokes")


def set_viscosity_law(th_space, law=None, temperature=None):
    """Attach a non-Newtonian law to a Taylor-Hood space (fs_space_set_viscosity_law): law = None detaches; (p_ref, exponent):
    nu (p / p_ref)^exponent; ('pT', p_ref, c_p, T_ref, c_T) with temperature = DeviceVector of the CG1 vertex values (local
    numbering; read at every assembly, so the caller keeps it alive and current): nu (1 + c_p p/p_ref)(1 - c_T T/T_ref)."""
    f = L.fs_viscosity_law()
    if law is not None and law[0] == 'pT':
        if temperature is None:
            raise BackendError("set_viscosity_law: the 'pT' law needs the temperature vector")
        f.kind, f.pressure_ref, f.pressure_coef, f.temperature_ref, f.temperature_coef = 2, float(law[1]), float(law[2]), float(law[3]), float(law[4])
        f.temperature = temperature.h.value
        th_space._law_temperature = temperature
    elif law is not None:
        f.kind, f.pressure_ref, f.pressure_exponent = 1, float(law[0]), float(law[1])
    L.check(L.load().fs_space_set_viscosity_law(th_space.h, C.byref(f) if law is not None else None), "fs_space_set_viscosity_law")
    if law is None or law[0] != 'pT':
        th_space._law_temperature = None


def assemble_ns_pressure_boundary(J, g, facet_cell, facet_opposite, nu, facet_value=None, viscosity_law=None, w0=None):
    """J, g += p_b n.v ds - nu ((grad u + grad u^T) n).v ds on the listed boundary facets (value None: traction term only;
    a number, one value per facet, or [n_facets, 3] values at the facet's vertices in the cell's local order).
    viscosity_law = (p_ref, exponent) with the state w0: nu (p0 / p_ref)^exponent."""
    fc = np.ascontiguousarray(facet_cell, dtype=np.int32)
    fo_ = np.ascontiguousarray(facet_opposite, dtype=np.int32)
    fv, per = None, 1
    if facet_value is not None:
        a = np.asarray(facet_value, dtype=np.float64)
        if a.ndim == 2 and a.shape[0] == len(fc) and a.shape[1] in (2, 3):       # values at the vertices of every facet (edge: 2)
            fv, per = np.ascontiguousarray(a), a.shape[1]
        else:
            fv = np.ascontiguousarray(np.broadcast_to(a, fc.shape))
    pref, ex = (0.0, 0.0) if viscosity_law is None else (float(viscosity_law[0]), float(viscosity_law[1]))
    L.check(L.load().fs_assemble_ns_pressure_boundary_nn(J.h, g.h, len(fc), L.p_i32(fc), L.p_i32(fo_), L.p_f64(fv), float(nu),
                                                         w0.h if w0 is not None else None, pref, ex, per),
            "fs_assemble_ns_pressure_boundary")


def saddle_solve(J, Kp, Mp, b, x, nu, rho=1.0, inv_dt=0.0, rtol=1e-8, atol=0.0, max_iter=0, restart=0,
                 velocity_sweeps=0, inner_rtol=0.0, nonzero_guess=False, Kp_amg=None):
    """FGMRES with the block-triangular Cahouet-Chabard preconditioner; Kp may be None for steady problems."""
    o = L.fs_saddle_opts()
    o.rtol, o.atol, o.max_iter, o.restart = float(rtol), float(atol), int(max_iter), int(restart)
    o.kinematic_viscosity, o.density, o.inv_dt = float(nu), float(rho), float(inv_dt)
    o.velocity_sweeps, o.inner_rtol, o.nonzero_guess = int(velocity_sweeps), float(inner_rtol), 1 if nonzero_guess else 0
    st = L.fs_krylov_stats()

    def solve():
        L.check(L.load().fs_saddle_solve(J.h, Kp.h if Kp is not None else None, Kp_amg.h if Kp_amg is not None else None,
                                         Mp.h, b.h, x.h, C.byref(o), C.byref(st)),
                "fs_saddle_solve")
    _with_p2p_fallback([M.space for M in (J, Kp, Mp) if M is not None], solve, x if nonzero_guess else None)
    return {k: getattr(st, k) for k, _ in L.fs_krylov_stats._fields_}


def assemble_large_deformation(J, rhs, u, w, u0, w0, dt, q, mu, lmbda, dirichlet, body_force=(0.0, 0.0, 0.0), facet_cell=None,
                               facet_opposite=None, facet_g=None):
    """Reduced Newton system of one Crank-Nicolson step of large-deformation elasticity (fs_assemble_large_deformation): J and rhs
    on the CG1 block-4 space, u / u0 vector CG1 dof vectors, w / w0 block vectors (v, p).  dirichlet: uint8 per vertex (bits 0-2
    displacement, 3-5 velocity, 6 pressure).  Facets (device cells, local opposite vertex, g [nf, 3]) carry follower loads.
    Returns {'residual_norm', 'n_bad', 'first_bad_cell'}."""
    f = L.fs_ld_form()
    f.dt, f.q, f.mu, f.lambda_ = float(dt), float(q), float(mu), float(lmbda)
    for i, x in enumerate(tuple(body_force)[:3]):
        f.body_force[i] = float(x)
    dm = np.ascontiguousarray(dirichlet, dtype=np.uint8)
    f.dirichlet = dm.ctypes.data
    keep = [dm]
    if facet_cell is not None and len(facet_cell):
        fc, fo = L.i32(facet_cell), L.i32(facet_opposite)
        g = np.zeros((len(fc), 3))
        gg = np.asarray(facet_g, dtype=np.float64).reshape(len(fc), -1)
        g[:, :gg.shape[1]] = gg
        keep += [fc, fo, g]
        f.n_facets, f.facet_cell, f.facet_opposite, f.facet_g = len(fc), fc.ctypes.data, fo.ctypes.data, g.ctypes.data
    info = L.fs_ld_info()
    L.check(L.load().fs_assemble_large_deformation(J.h, rhs.h, u.h, w.h, u0.h, w0.h, C.byref(f), C.byref(info)),
            "fs_assemble_large_deformation")
    del keep
    return {"residual_norm": info.residual_norm, "n_bad": int(info.n_bad), "first_bad_cell": int(info.first_bad_cell)}


def large_deformation_solve(J, Mp, b, x, a0, schur_scale, a0_amg=None, a0_rtol=0.0, rtol=1e-10, atol=0.0, max_iter=0, restart=0,
                            nonzero_guess=False):
    """FGMRES of fs_saddle_solve on the reduced large-deformation operator, right-preconditioned by the block upper triangular
    [A J_vp; 0 S]^-1: S = schur_scale * Mp, A^-1 one V-cycle of a0_amg or Jacobi-CG on a0 to a0_rtol.  nonzero_guess: x holds the
    starting vector (else it is zeroed), as in saddle_solve."""
    o = L.fs_saddle_opts()
    o.rtol, o.atol, o.max_iter, o.restart = float(rtol), float(atol), int(max_iter), int(restart)
    o.block_upper, o.a0, o.a0_rtol, o.schur_scale = 1, a0.h, float(a0_rtol), float(schur_scale)
    o.nonzero_guess = 1 if nonzero_guess else 0
    o.a0_amg = a0_amg.h if a0_amg is not None else None
    st = L.fs_krylov_stats()
    L.check(L.load().fs_saddle_solve(J.h, None, None, Mp.h, b.h, x.h, C.byref(o), C.byref(st)), "fs_saddle_solve")
    return {k: getattr(st, k) for k, _ in L.fs_krylov_stats._fields_}


def saddle_last_cycle():
    """The state of the last FGMRES cycle of the most recent saddle_solve / large_deformation_solve call (fs_saddle_last_cycle, a
    test / inspection hook), or None when that call ran no cycle.  m: restart length; kuse: columns used; V [kuse + 1, n], Z [kuse, n]
    (owned rows); R [m + 1, m]: the rotated Hessenberg matrix; cs, sn [m]; gamma [m + 1]; y [m]: the least-squares solution (the device
    keeps its negative); second_passes; vel_lmax.  Column kuse of R and entry kuse of cs, sn may hold an iteration that was enqueued ahead
    and never used; it has then rotated gamma[kuse] on into gamma[kuse + 1] (include/fenicssolver_amd.h)."""
    lib = L.load()
    info = L.fs_saddle_cycle_info()
    rc = lib.fs_saddle_last_cycle(C.byref(info), None, None, None, None, None, None, None)
    if rc == L.FS_ERR_UNSUPPORTED:
        return None
    L.check(rc, "fs_saddle_last_cycle")
    m, k, n = info.restart, info.columns_used, info.n_owned
    V, Z, H = np.empty((k + 1, n)), np.empty((k, n)), np.empty((m + 1, m))
    cs, sn, gam, y = np.empty(m), np.empty(m), np.empty(m + 1), np.empty(m)
    L.check(lib.fs_saddle_last_cycle(C.byref(info), L.p_f64(V), L.p_f64(Z) if k else None, L.p_f64(H), L.p_f64(cs), L.p_f64(sn),
                                     L.p_f64(gam), L.p_f64(y)), "fs_saddle_last_cycle")
    return {"m": m, "kuse": k, "V": V, "Z": Z, "R": H, "cs": cs, "sn": sn, "gamma": gam, "y": -y,
            "second_passes": info.second_passes, "vel_lmax": info.vel_lmax}


def krylov_history():
    n = C.c_int(0)
    L.load().fs_krylov_history(None, 0, C.byref(n))
    out = np.empty(max(n.value, 1))
    L.load().fs_krylov_history(L.p_f64(out), n.value, C.byref(n))
    return out[: n.value]


# ---- multi-GPU ------------------------------------------------------------------------------
def comm_unique_id():
    buf = C.create_string_buffer(L.FS_UNIQUE_ID_BYTES)
    L.check(L.load().fs_comm_get_unique_id(buf), "fs_comm_get_unique_id")
    return bytes(buf.raw)


_comm_up = False


def comm_init(n_ranks, rank, uid):
    global _comm_up
    L.check(L.load().fs_comm_init(int(n_ranks), int(rank), C.c_char_p(uid)), "fs_comm_init")
    _comm_up = True


def comm_info():
    """(n_ranks, rank) of the communicator that is up ((1, 0) without one)."""
    n, r = C.c_int(1), C.c_int(0)
    L.check(L.load().fs_comm_info(C.byref(n), C.byref(r)), "fs_comm_info")
    return n.value, r.value


def comm_finalize():
    global _comm_up
    L.check(L.load().fs_comm_finalize(), "fs_comm_finalize")
    _comm_up = False


def comm_allreduce_sum(values):
    v = L.f64(values).ravel().copy()
    L.check(L.load().fs_comm_allreduce_sum(L.p_f64(v), v.size), "fs_comm_allreduce_sum")
    return v


def comm_allgather(values, n_max):
    """[n_ranks, n_max]: every rank's values (padded to n_max), one ncclAllGather."""
    v = L.f64(values).ravel()
    n_ranks = comm_info()[0]
    out = np.empty((n_ranks, int(n_max)))
    L.check(L.load().fs_comm_allgather(L.p_f64(v), v.size, int(n_max), L.p_f64(out)), "fs_comm_allgather")
    return out


def halo_exchange(space, v):
    L.check(L.load().fs_halo_exchange(space.h, v.h), "fs_halo_exchange")


def comm_benchmark(space, reps=200):
    """(allreduce_ms, halo_ms): mean latency of the 3-double all-reduce and of this space's ghost refresh, as a CG
    iteration issues them.  Collective (every rank calls it); zeros on one rank."""
    a, h = C.c_double(), C.c_double()
    L.check(L.load().fs_comm_benchmark(space.h, int(reps), C.byref(a), C.byref(h)), "fs_comm_benchmark")
    return a.value, h.value


def last_product_kind():
    """Kernel family of the last product this process launched (fs_last_product_kind): 0 streaming, 1 row-dictionary work items,
    2 lattice tiles (CG2 box), 3 marching windows (P1 box), 4 block-row dictionary, 5 marching windows (CG2 box in lattice order)."""
    return int(L.load().fs_last_product_kind())


def last_iteration_form():
    """Form of the one-launch CG iteration in the last solve (fs_last_iteration_form), 0 if it did not run: bit 0 = p and x updated every
    second launch (option "cg_pair"), bit 1 = dot weights from the table by row class."""
    return int(L.load().fs_last_iteration_form())


def last_iteration_guard():
    """What option "cg_guard" did in the last solve (fs_last_iteration_guard), 0 if nothing: bit 0 = guarded work vectors without the
    edge-item path, bit 1 = own rows from the centre run (Kuhn box)."""
    return int(L.load().fs_last_iteration_guard())


def last_iteration_runs():
    """How many of a Kuhn-box row's seven runs the one-launch CG iteration of the last solve left out because every row class of the
    operator held nothing above 2^-53 of its unit diagonal there (fs_last_iteration_runs, option "cg_zero_runs"): 0 or 2."""
    return int(L.load().fs_last_iteration_runs())


def set_option(name, value):
    L.check(L.load().fs_set_option(name.encode(), float(value)), "fs_set_option")


# ---- DG1 (ScalarTransportDGSolver) -------------------------------------------------------------------------------------------
class DeviceDGSpace(_Handle):
    """Discontinuous P1 scalar space on a device mesh: dof (K, a) = (d+1) K + a in device cell order (fs_space_create with
    FS_FAMILY_DG).  plus_key: one int64 per device cell; on every interior facet the cell with the larger key is '+'."""
    _destroy = "fs_space_destroy"

    def __init__(self, mesh, plus_key=None):
        super().__init__()
        self.mesh = mesh
        L.check(L.load().fs_space_create(mesh.h, L.FS_FAMILY_DG, 1, 1, C.byref(self.h)), "fs_space_create(DG)")
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.load().fs_space_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "fs_space_info")
        self.n_local, self.n_owned, self.nnz, self.stored_values = a.value, b.value, c.value, d.value
        self.ncomp = 1
        if plus_key is not None:
            self.set_plus_key(plus_key)

    def set_plus_key(self, key):
        k = L.i64(key).ravel()
        L.check(L.load().fs_space_dg_set_plus_key(self.h, L.p_i64(k)), "fs_space_dg_set_plus_key")


class DeviceDGMatrix(DeviceMatrix):
    """Cell-block matrix of a DG1 space: (d+2) blocks of (d+1)^2 values per cell (fs_matrix_create on a DG space)."""

    def assemble_transport(self, b=None, conductivity=0.0, capacity=1.0, velocity=(0.0, 0.0, 0.0), alpha=0.0, operator_scale=1.0,
                           mass_scale=0.0, facet_cell=None, facet_local=None, facet_h=None, facet_g=None, source=None, add=False):
        """fs_assemble_dg_transport: A (and b) <- operator_scale c a(T, v) + mass_scale M + the listed boundary facets' HTC
        mass facet_h; b <- int source v dx + int g v ds.  Facets, source: device cell numbering."""
        f = L.fs_dg_form()
        f.conductivity, f.capacity, f.alpha = float(conductivity), float(capacity), float(alpha)
        v = np.zeros(3)
        v[:len(velocity)] = np.asarray(velocity, dtype=np.float64)
        f.velocity[:] = list(v)
        f.operator_scale, f.mass_scale = float(operator_scale), float(mass_scale)
        keep = []
        if facet_cell is not None and len(facet_cell):
            fc, fl = L.i32(facet_cell).ravel(), L.i32(facet_local).ravel()
            keep += [fc, fl]
            f.n_facets, f.facet_cell, f.facet_local = fc.size, L.p_i32(fc), L.p_i32(fl)
            if facet_h is not None:
                fh = L.f64(np.broadcast_to(facet_h, (fc.size,)))
                keep.append(fh)
                f.facet_h = L.p_f64(fh)
            if facet_g is not None:
                fg = L.f64(facet_g).reshape(fc.size, -1)
                keep.append(fg)
                f.facet_g = L.p_f64(fg)
        if source is not None:
            src = L.f64(source)
            keep.append(src)
            f.source = L.p_f64(src)
        f.add = 1 if add else 0
        L.check(L.load().fs_assemble_dg_transport(self.h, b.h if b is not None else None, C.byref(f)), "fs_assemble_dg_transport")

    def apply_dirichlet(self, b, dofs, vals, symmetric=False):
        if symmetric:
            raise BackendError("DG matrices take Dirichlet rows as identity rows (symmetric=False)")
        DeviceMatrix.apply_dirichlet(self, b, dofs, vals, symmetric=False)


def dg_krylov_solve(A, b, x, rtol=1e-12, atol=0.0, max_iter=20000, precond="block_jacobi", batch=0, nonzero_guess=False,
                    norm="preconditioned"):
    """BiCGStab on a DG1 cell-block matrix, right-preconditioned by the inverse diagonal blocks ("block_jacobi"), the inverse
    diagonal ("jacobi") or nothing ("none").  norm: "preconditioned" stops when ||r|| <= rtol ||b|| and ||M^-1 r|| <= rtol ||M^-1 b||
    both hold, "unpreconditioned" on the first alone (the stats' residuals are in the plain norm); converged = 1 means the TRUE
    residual met the test.
    Returns the stats dict of fs_krylov_solve."""
    o = L.fs_krylov_opts()
    o.method = L.FS_KSP_BICGSTAB
    o.precond = {"block_jacobi": L.FS_PC_BLOCK_JACOBI, "jacobi": L.FS_PC_JACOBI, "none": L.FS_PC_NONE, None: L.FS_PC_NONE}[precond]
    o.rtol, o.atol, o.max_iter, o.batch = float(rtol), float(atol), int(max_iter), int(batch)
    o.nonzero_guess = 1 if nonzero_guess else 0
    o.norm_type = {"unpreconditioned": L.FS_NORM_UNPRECONDITIONED, "preconditioned": L.FS_NORM_PRECONDITIONED}[norm]
    st = L.fs_krylov_stats()
    rc = L.load().fs_krylov_solve(A.h, b.h, x.h, C.byref(o), C.byref(st))
    out = {k: getattr(st, k) for k, _ in L.fs_krylov_stats._fields_}
    L.check(rc, "fs_krylov_solve(DG)")
    return out


def assemble_dg_projection(dg_space, x, cg1_space, b):
    """b_i = int T_h phi_i dx of the DG1 field x on the CG1 space of the same device mesh (fs_assemble_dg_projection)."""
    L.check(L.load().fs_assemble_dg_projection(dg_space.h, x.h, cg1_space.h, b.h), "fs_assemble_dg_projection")
