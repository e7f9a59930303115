/*
 * fenicssolver_amd.h — C-ABI of libfsamd.so, the MI355X (gfx950) replacement for
 * the part of FenicsSolver that the reference delegates to DOLFIN/FFC/PETSc.
 *
 * The reference has no FFI of its own: the seam is the Python methods
 *   SolverBase.solve_linear_problem(F, u, bcs)   FenicsSolver/SolverBase.py:592-613
 *   SolverBase.solve_amg(F, u, bcs)              FenicsSolver/SolverBase.py:643-672
 *   SolverBase.solve_nonlinear_problem(...)      FenicsSolver/SolverBase.py:615-626
 * which call dolfin.assemble / assemble_system / DirichletBC.apply /
 * LinearVariationalSolver / PETScKrylovSolver.  Each entry point below names the
 * dolfin call (and the reference line that makes it) that it stands in for; the
 * ctypes binding a maintainer would add is fenicssolver_amd/_lib.py (see
 * INTEGRATION.md).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no exceptions cross the boundary.
 *   - every function returns 0 (FS_OK) or a negative FS_ERR_* code; the message is
 *     available from fs_last_error() (thread-local).
 *   - handles are opaque and own device (HBM) memory; host arrays passed in are
 *     borrowed for the duration of the call only (C-contiguous, fp64 / int32 / int64).
 *   - calls are synchronous at return unless stated otherwise.
 *   - one process drives one GPU; N-GPU runs are N processes joined through
 *     fs_comm_init (RCCL).  All field arithmetic is fp64, connectivity is int32.
 *   - threading: one thread at a time per process, as for the PETSc objects of one communicator.  All work is
 *     ordered on the library's single HIP stream, the device block cache and the Krylov / AMG / saddle-point work
 *     spaces (and fs_krylov_history) belong to the process.  The three solve entry points (fs_krylov_solve, fs_amg_solve,
 *     fs_saddle_solve) take a process-wide lock and the block cache its own, so concurrent calls from several threads are
 *     serialised, not undefined; assembly calls on DIFFERENT handles may overlap on the host but still share the stream.
 *     Concurrency comes from running one process per GPU.
 */
#ifndef FENICSSOLVER_AMD_H
#define FENICSSOLVER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FS_OK 0
#define FS_ERR_INVALID (-1)   /* bad argument / handle */
#define FS_ERR_HIP (-2)       /* HIP runtime error (message has the hipError string) */
#define FS_ERR_NO_DEVICE (-3) /* no gfx950 device visible: the library never falls back to the CPU */
#define FS_ERR_UNSUPPORTED (-4)
#define FS_ERR_COMM (-5)      /* RCCL error */
#define FS_ERR_NUMERIC (-6)   /* Krylov breakdown (non-SPD operator, NaN) */
#define FS_ERR_P2P_TIMEOUT (-7) /* a wait of the peer-to-peer halo exchange timed out (FS_P2P_TIMEOUT_MS): the transport failed, not the solve;
                                 * the host side turns the exchange of the space off on every rank and solves again over RCCL */

typedef struct fs_mesh_s* fs_mesh_t;
typedef struct fs_space_s* fs_space_t;
typedef struct fs_matrix_s* fs_matrix_t;
typedef struct fs_vector_s* fs_vector_t;

/* ---- runtime ---------------------------------------------------------------- */

/* Select the HIP device this process drives (dolfin has no analogue; MPI rank ->
 * device mapping replaces `mpirun`, SolverBase.py:102-118).  Also loads the library's code objects onto the device (about 70 ms,
 * half of it the set-up kernels' object with its rocPRIM sorts) so that the first mesh, space and solve of the process do not pay
 * for it; environment FS_PRELOAD=0 leaves the loading to the first launch out of each object.
 * Other environment switches read once per process (A/B and fall-backs, not needed for normal use): FS_PATTERN_BY_ROWS=0 (CG1
 * sparsity patterns through sorted node-pair keys instead of row by row), FS_DICT_REUSE=0 (row classes found from scratch at every
 * solve instead of compared with the kept table), FS_CG_FUSED / FS_CG_FUSED_MAX_ROWS / FS_CG_FUSED_P2P (the one-launch CG
 * iteration: option "cg_fused"), FS_SPMV_DICT=0 (no row-dictionary product: option "row_dictionary"). */
int fs_init(int device_id);
int fs_device_count(int* count);
int fs_device_synchronize(void);
/* Enqueues an empty kernel named k_profile_marker on the library's stream (no dolfin analogue; the reference's only timing is the
 * wall clock around solve(), SolverBase.py:514-525).  A traced command (rocprofv3 --kernel-trace / --pmc) that runs several problem
 * sizes or kernel variants back to back calls it between them; the n-th marker opens phase n of tools/summarize_profiles.py. */
int fs_profile_marker(int phase);
/* Device blocks released by the library are cached for re-use (hipFree synchronises the device, a time loop that
 * re-assembles its operators must not pay it every step): fs_memory_info reports the bytes in use / idle in the
 * cache, fs_memory_trim returns the idle ones to the driver.  FS_POOL_MAX_MB (environment, default 16384) caps the
 * idle bytes; 0 turns the cache off. */
int fs_memory_info(int64_t* live_bytes, int64_t* cached_bytes);
int fs_memory_trim(void);
const char* fs_last_error(void);
const char* fs_version(void);
/* Tunables: "spmv_blocks" (persistent SpMV grid, multiple of 8), "spmv_unroll"
 * (2/4/8/16 row entries in flight per lane), "spmv_unroll4" (1/2/4: the same for 4 x 4 block rows), "cg_batch" (iterations per host poll), "lattice_order" (-1 / 0 / 1: scalar CG2 operators on uniform boxes solved in
 * the lattice order of the half grid, fs_krylov_stats.lattice_order - automatic = from 270 000 rows on, where the product is then the
 * marching-window product k_lat_march or the tile product k_lattice_spmv / never / wherever the order exists), "lattice_march" (1 / 0, round 6: k_lat_march where
 * its tables can be built - every class inside its parity's compile-time stencil, every mesh line of one class per parity away from its ends - / the tile product; the same bits),
 * "lattice_check" (0 / 1: every solve in lattice order first compares that product with the work-item product on a
 * vector of pseudo-random numbers, every row, bit for bit - a difference fails the solve with FS_ERR_NUMERIC), "cg_mirror" (0 / 1: the one-launch iteration reports its progress
 * through pinned host memory and the host keeps "cg_ahead" to "cg_ahead" + "cg_sub" launches enqueued, instead of batches of
 * "cg_batch" with the status word copied back behind each),
 * "cg_fuse_sums" (0/1: sum the dot partials inside the update kernel on one GPU),
 * "update_blocks" (grid of the fused vector-update kernel, 1 to 2048: every workgroup leaves dot partials in a fixed buffer), "cg_graph" (-1 / 0 / 1: CG batches as hipGraphs by size /
 * never / always), "cg_fused" (-1 / 0 / 1: ONE launch per CG iteration on row-dictionary operators - up to 3 M rows /
 * never / wherever it applies; fs_krylov_stats.fused_iteration), "cg_pair" (1 / 0, default 1; FS_CG_PAIR in the environment: that launch
 * updates p and x every second iteration, two steps in one pass, instead of in every launch - the same bits; fs_last_iteration_form),
 * "cg_guard" (1 / 0, default 1; FS_CG_GUARD in the environment: on one GPU the LIGHT / PAIR launches of "cg_pair" run on solver-owned work vectors with
 * guard bands of zeros in front of row 0 and behind the last row, so that no work item needs the clamped edge path, and on a Kuhn box take a lane's
 * own rows from the centre run instead of a run of their own - the same bits; fs_last_iteration_guard; 0: unguarded vectors and the kernels with the edge path),
 * "cg_zero_runs" (-1 / 0 / 1, default -1; FS_CG_ZERO_RUNS in the environment: on a Kuhn box those launches neither load nor multiply the two runs of a row in which no
 * row class of the scaled operator holds a coefficient above 2^-53 - the (0, 1, 1) and (1, 1, 1) diagonals of a pure diffusion operator on orthogonal edges, where the
 * assembly leaves the rounding of sums that cancel; iterates equal to rounding, not bit for bit - from "cg_zero_runs_min_rows" rows on (default and floor 100 000) / never /
 * wherever it applies; fs_last_iteration_runs), "cg_poison_p" (tests: 1 = the next CG solve
 * finds NaN in its search-direction workspace before it sets its initial state), "row_dictionary" (0 / 1: allow the row-dictionary form of the product, fs_krylov_stats.row_classes),
 * "box_snap" (0 / 1: box meshes snap their edge vectors to the grid spacing so that equal stencils are equal bit for bit),
 * "box_assembly" (1 / 0: scalar CG1 operators on fs_mesh_create_box meshes are assembled from the reference rows of the six cell types instead of
 * per-incidence geometry - the same bits), "box_spmv" (1 / 0) and "box_min_rows" (default 1 500 000): the marching-window product k_box_spmv,
 * "box_iter" (0 / 1, default 0: opt-in) and "box_iter_min_rows" (default 400 000): the one-launch CG iteration of P1 box operators in marching-window
 * form (k_box_cg_iter; iterates equal to the other forms to rounding, not bit for bit; measured slower than k_dict_cg_iter up to 3 M rows),
 * "amg_coarse_fp32" (1 / 0, default 1: hierarchies built from now on keep the 6 x 6-block coarse operators and the transfer operators
 * the V-cycle streams rounded to fp32 - vectors, accumulation, the fine level and the CG outside stay fp64; fs_amg_level_get keeps
 * returning the fp64 operators; FS_AMG_FP32=0 in the environment is the same switch). */
int fs_set_option(const char* name, double value);
/* Name, CU count and HBM bytes of the selected device. */
int fs_device_info(char* name, int name_len, int* compute_units, int64_t* hbm_bytes);

/* ---- mesh  (dolfin.Mesh / BoxMesh, SolverBase.py:203-258) -------------------- */

/* Upload a tetrahedral mesh (gdim 3, 4 vertices per cell) or a triangular mesh (gdim 2, 3 vertices per
 * cell: scalar CG1 spaces, one GPU; facet lists of the boundary calls are then [n_facets][2] edge vertex pairs).
 * xyz[nv][gdim], cells[nc][verts_per_cell] vertex indices.  The first n_owned vertices are the rows this process owns
 * (n_owned == nv on one GPU); the remainder are ghost vertices whose values
 * arrive by halo exchange. */
int fs_mesh_create(int gdim, int64_t nv, const double* xyz, int64_t nc, const int32_t* cells,
                   int verts_per_cell, int64_t n_owned, fs_mesh_t* out);

/* Generate on the device the slab of dolfin.BoxMesh(p0, p1, nx, ny, nz) whose
 * owned vertex planes are [zplane_begin, zplane_end) (0 .. nz+1 for the whole
 * mesh).  Vertex order x-fastest, six tets per hex around the v0-v7 diagonal,
 * cells iz->iy->ix, each cell's vertices ascending by global index (SURVEY.md
 * section 8d / Appendix D-8).  Local numbering: owned planes first, then the
 * lower ghost plane, then the upper ghost plane. */
int fs_mesh_create_box(int64_t nx, int64_t ny, int64_t nz, const double p0[3], const double p1[3],
                       int64_t zplane_begin, int64_t zplane_end, fs_mesh_t* out);

/* Global vertex ids of an uploaded mesh part (identity by default).  Needed for CG2 spaces on a decomposed mesh:
 * an edge node is owned by the rank owning its endpoint of smaller global id. */
int fs_mesh_set_global_ids(fs_mesh_t mesh, const int64_t* global_ids);
int fs_mesh_info(fs_mesh_t mesh, int64_t* nv, int64_t* nc, int64_t* n_owned);
/* Copy back to host (any pointer may be NULL): xyz[nv][3], cells[nc][4],
 * global vertex ids[nv] (identity for uploaded meshes). */
int fs_mesh_get(fs_mesh_t mesh, double* xyz, int32_t* cells, int64_t* global_ids);
int fs_mesh_destroy(fs_mesh_t mesh);
/* Locality order of a mesh that arrives in file order (DOLFIN reorders the dofs of every FunctionSpace when it builds
 * the dofmap, SolverBase.py:260-275): vertex_order[k] = the vertex to upload k-th (Morton curve of the coordinates),
 * cell_order[k] = the cell to upload k-th (by the smallest new index of its vertices, file order among equals).  Computed
 * on the device; host arrays in, host arrays out; nothing is created.  The caller uploads xyz[vertex_order] and the
 * re-indexed cells[cell_order] through fs_mesh_create and keeps the permutation to translate indices and results. */
int fs_mesh_locality_order(int gdim, int64_t nv, const double* xyz, int64_t nc, const int32_t* cells, int verts_per_cell,
                           int32_t* vertex_order, int32_t* cell_order);
/* fs_mesh_locality_order + fs_mesh_create in one: the tetrahedral mesh of a FILE (Mesh(filename), SolverBase.py:203-258) uploaded
 * once, ordered on the device, and built there in that order - coordinates gathered, cells gathered and renamed, the vertices'
 * global ids = their numbers in the file.  vertex_order[k] / cell_order[c] = file number of new vertex k / new cell c, for the
 * host's maps between file numbering (what the API speaks) and device numbering. */
int fs_mesh_create_renumbered(int64_t nv, const double* xyz, int64_t nc, const int32_t* cells, int32_t* vertex_order,
                              int32_t* cell_order, fs_mesh_t* out);

/* ---- function space + sparsity (dolfin.FunctionSpace, SolverBase.py:260-275;
 *      the sparsity pattern DOLFIN builds inside the first assemble()) --------- */

#define FS_FAMILY_CG 0
/* Discontinuous P1 (ScalarTransportDGSolver.py): degree 1, ncomp 1, one rank.  Dof (K, a) = (d+1) K + a in device cell order (a: the
 * cell's local vertex).  The space holds the cell-facet adjacency (the cell across the facet opposite every local vertex), the '+'
 * side of every interior facet (fs_space_dg_set_plus_key) and the vertex-to-cell incidences of the projection onto CG1.  Its matrices
 * are cell blocks (fs_assemble_dg_transport); fs_space_info reports n_dofs_local = n_dofs_owned = (d+1) n_cells and the stored
 * values as nnz / sell_entries. */
#define FS_FAMILY_DG 1
/* degree 1 with ncomp = 1 (scalar) or 3 (vector, node-interleaved dofs as DOLFIN's
 * VectorFunctionSpace lays them out; 2 on triangular meshes: plane-strain elasticity); triangular meshes also carry
 * degree-2 spaces, scalar or 2-vector (3 vertices + 3 edge nodes per cell, UFC edge i opposite vertex i); degree 2 with ncomp = 1 (scalar) or 4 (Taylor-Hood block u_x,u_y,u_z,p); degree 1 with ncomp = 4 (the (v_x,v_y,v_z,p) block of fs_assemble_large_deformation, one per vertex):
 * nodes = the vertices, then one node per edge, edges numbered lexicographically by their ascending vertex
 * pair - grouped by index difference first on structured meshes.  With ghost vertices
 * (n_owned < nv) the nodes are [owned vertices | owned edges | ghost vertices | ghost edges]; an edge belongs to
 * the rank owning its endpoint of smaller global id (fs_mesh_set_global_ids). */
int fs_space_create(fs_mesh_t mesh, int family, int degree, int ncomp, fs_space_t* out);
/* The same space with additional node couplings in the sparsity pattern (node_pairs [n_pairs][2], both directions are
 * added): what DOLFIN's pattern builder does for a form with interior-facet (dS) integrals, where the two vertices
 * opposite a facet couple although they share no cell (ScalarTransportSolver.py:312-315), and for a periodic space, whose
 * folded system (fs_matrix_tie_nodes) couples every master with the neighbours of its slave.  CG1 and CG2. */
int fs_space_create_coupled(fs_mesh_t mesh, int family, int degree, int ncomp, int64_t n_pairs, const int32_t* node_pairs,
                            fs_space_t* out);
int fs_space_info(fs_space_t space, int64_t* n_dofs_local, int64_t* n_dofs_owned, int64_t* nnz,
                  int64_t* sell_entries);
/* DG spaces: which cell of an interior facet is its '+' side (DOLFIN's interior-facet assembler, the restriction ('+') of h in
 * ScalarTransportDGSolver.py): the one with the larger key[cell] (device cell order).  Without a call the key is minus the caller's
 * cell number (the lower caller number is '+'); a caller with cell-region markers passes marker * n_cells - caller number. */
int fs_space_dg_set_plus_key(fs_space_t space, const int64_t* key);
/* A += coefficient * avg(h)^2 jump(grad u, n) jump(grad v, n) dS over the listed interior facets, h = 2 circumradius
 * (the 'IP' stabilisation of ScalarTransportSolver.py:312-315, coefficient = alpha * capacity).  facet_cells
 * [n_facets][2]: the two local cells of every facet.  Scalar CG1 on tetrahedra, space from fs_space_create_coupled. */
int fs_assemble_interior_penalty(fs_matrix_t A, int64_t n_facets, const int32_t* facet_cells, double coefficient);

/* Storage form chosen per 64-row slice: SELL (values + 4-B columns) or DIA (values only, the
 * 64 rows share one list of column offsets).  spmv_bytes = matrix bytes one SpMV streams. */
int fs_space_format_info(fs_space_t space, int64_t* n_slices, int64_t* n_dia_slices, int64_t* spmv_matrix_bytes);
/* CG2: the edge table [n_edges][2] (edge node e is dof n_vertices + e); n_edges = 0 for CG1. */
int fs_space_get_edges(fs_space_t space, int64_t* n_edges, int32_t* edges);
int fs_space_destroy(fs_space_t space);

/* ---- vectors (dolfin.Function.vector(), PETScVector) ------------------------ */

int fs_vector_create(int64_t n, fs_vector_t* out);
int fs_vector_size(fs_vector_t v, int64_t* n);
int fs_vector_set(fs_vector_t v, const double* host, int64_t n);
int fs_vector_get(fs_vector_t v, double* host, int64_t n);
int fs_vector_fill(fs_vector_t v, double value);      /* enqueued on the library's stream: returns without waiting for the kernel */
int fs_vector_axpy(fs_vector_t y, double a, fs_vector_t x); /* y += a x */
int fs_vector_copy(fs_vector_t dst, fs_vector_t src, int64_t n); /* first n entries, device to device (Function.assign) */
/* v[idx[k]] += vals[k] (repeated indices accumulate): dolfin.PointSource.apply(b), SolverBase.py:597-601 */
int fs_vector_add_entries(fs_vector_t v, int64_t n, const int32_t* idx, const double* vals);
int fs_vector_dot(fs_vector_t x, fs_vector_t y, double* result); /* local (un-reduced) dot */
int fs_vector_destroy(fs_vector_t v);

/* ---- matrices (PETSc AIJ behind dolfin.assemble, SolverBase.py:595, 608-612, 644) */

/* A matrix on the space's sparsity pattern, values zero.  Rows = owned dofs,
 * columns = local (owned + ghost) dofs.  On a DG space: (d+2) blocks of (d+1) x (d+1) values per cell - slot 0 the diagonal block,
 * slot k+1 the coupling with the cell across facet k - stored with the cell index fastest.  DG matrices are accepted by
 * fs_matrix_info, fs_matrix_zero, fs_matrix_get_csr (dof order, the zero blocks of boundary facets left out), fs_apply_dirichlet
 * (symmetric = 0), fs_spmv, fs_krylov_solve (BiCGStab) and fs_assemble_dg_transport; every other entry point returns
 * FS_ERR_UNSUPPORTED for them. */
int fs_matrix_create(fs_space_t space, fs_matrix_t* out);
int fs_matrix_info(fs_matrix_t A, int64_t* n_rows, int64_t* n_cols, int64_t* nnz);
int fs_matrix_zero(fs_matrix_t A);
/* Y += a X (same space). Used for theta-scheme operators M/dt + theta K
 * (ScalarTransportSolver.py:287-293). */
int fs_matrix_axpy(fs_matrix_t Y, double a, fs_matrix_t X);
/* dst = src (same space), enqueued on the library's stream: a time loop with constant coefficients keeps its
 * unconstrained operator and starts every step from a copy (DOLFIN re-assembles, SolverBase.py:592-602). */
int fs_matrix_copy(fs_matrix_t dst, fs_matrix_t src);
/* Periodic constraints (FunctionSpace(..., constrained_domain=pb), SolverBase.py:260-275): node slaves[i] takes the
 * value of node masters[i] (chains resolved by the caller, a master is never a slave).  DOLFIN removes the slave dofs;
 * here the assembled system is folded in place - A <- P^T A P with a unit diagonal on the slave rows, b <- P^T b with 0
 * on the slaves (b may be NULL) - and after the solve fs_vector_assign_entries copies the masters' values to the
 * slaves.  The pattern must hold (master, j) and (master, fold(j)) for every neighbour j of a slave: create the space
 * with fs_space_create_coupled.  Apply before fs_apply_dirichlet.  Decomposed spaces: local node numbers, ghosts included -
 * the columns of every local slave fold onto its master in the rows this rank owns, the row of a slave folds on the rank that
 * owns it, which must own its master too. */
int fs_matrix_tie_nodes(fs_matrix_t A, fs_vector_t b, int64_t n_pairs, const int32_t* slaves, const int32_t* masters);
/* v[dst_nodes[i]*block + c] = v[src_nodes[i]*block + c], c < block. */
int fs_vector_assign_entries(fs_vector_t v, int64_t n, const int32_t* dst_nodes, const int32_t* src_nodes, int block);
/* Export as sorted-column CSR (any pointer may be NULL): rowptr[n_rows+1],
 * colidx[nnz], vals[nnz]. */
int fs_matrix_get_csr(fs_matrix_t A, int32_t* rowptr, int32_t* colidx, double* vals);
int fs_matrix_destroy(fs_matrix_t A);

/* Coefficient of a volume term: constant, one value per cell (DG0, e.g. a
 * per-subdomain material, SolverBase.py:331-332) or a constant 3x3 tensor
 * (as_matrix, SolverBase.py:327-330). */
#define FS_COEF_NONE 0
#define FS_COEF_CONST 1
#define FS_COEF_CELL 2
#define FS_COEF_TENSOR 3
#define FS_COEF_NODAL 4 /* linear forms only: P1-interpolated coefficient */
#define FS_COEF_CELL_TENSOR 6 /* stiffness only: data[n_cells][9], one row-major 3x3 tensor per cell (2-D: leading 2x2 block) -
                               * an Expression of degree 0 with a tensor value, examples/test_heat_transfer.py:90 */
#define FS_COEF_CELL_QP 7 /* stiffness on CG2 spaces only: data[n_cells][14], the coefficient at the 14 points of the degree-5 rule on
                           * tetrahedra / at the 6 points of the degree-4 rule on triangles (entries 0..5; the rest unused): a
                           * conductivity that depends on the P2 temperature iterate, evaluated where the integrand is */
#define FS_COEF_CELL_ROW 5 /* advection velocity only: data[n_cells][d+1][3], V_a = (d+1)/|K| int_K u phi_a dx per cell and test
                            * function - integrates inner(u, grad T) q dx exactly for a finite-element velocity u */
#define FS_COEF_CELL_LAME 8 /* fs_bilinear_form.lame only: data[n_cells][2], one (mu, lambda) pair per cell in device cell order -
                             * an isotropic material that varies from cell to cell (per-region E and nu) */

typedef struct fs_coef {
    int mode;             /* FS_COEF_* */
    double value;         /* FS_COEF_CONST */
    const double* data;   /* FS_COEF_CELL: [n_cells]; FS_COEF_NODAL: [n_dofs_local] (host) */
    double tensor[9];     /* FS_COEF_TENSOR, row-major */
} fs_coef;

/* Bilinear form  a(u,v) = int stiffness * grad u . grad v dx + int mass * u v dx
 * (scalar space: ScalarTransportSolver.py:284-285 and the 1/dt capacity term
 * :292), or for a vector space the isotropic elasticity operator
 * int (2 mu sym grad u + lambda div u I) : grad v dx  (LinearElasticitySolver.py:62-69, 215)
 * plus  mass * u . v.
 * Lame parameters: with lame.mode == FS_COEF_NONE (what a zero-initialised struct holds) the constants lame_mu / lame_lambda;
 * with lame.mode == FS_COEF_CELL_LAME, lame.data[n_cells][2] = (mu, lambda) per cell (host, device cell order) and lame_mu /
 * lame_lambda are ignored.  Per-cell pairs that all hold the constants give the constant operator bit for bit.  The atomic
 * P1 kernel (FS_ELASTICITY_ATOMIC) refuses per-cell pairs. */
typedef struct fs_bilinear_form {
    fs_coef stiffness;   /* scalar spaces */
    fs_coef mass;        /* both */
    double lame_mu;      /* vector spaces */
    double lame_lambda;  /* vector spaces */
    /* scalar spaces: + advection_scale * int (v . grad u) q dx  (ScalarTransportSolver.py:311; Galerkin,
     * non-symmetric).  v: FS_COEF_CONST -> tensor[0..2]; FS_COEF_CELL -> data[n_cells][3]; FS_COEF_CELL_ROW -> data[n_cells][d+1][3]. */
    fs_coef advection;
    double advection_scale;
    /* SUPG ("SPUG" in the reference, ScalarTransportSolver.py:259-270): the test function becomes
     * q + tau (v . grad q), tau = 0.5 h / (4/(Pe h) + 2|v|), h = 2 * circumradius of the cell.  supg_pe > 0 adds the
     * tau-part to the advection term (streamline diffusion) and to the mass term; v is the advection velocity
     * (set advection_scale = 0 to get the mass part only, e.g. for the old-step operator).  CG1 and CG2 scalar spaces; on CG2 the
     * diffusion term changes too: grad(q + tau v . grad q) = grad q + tau H_q v with the cell-wise constant Hessian of q. */
    double supg_pe;
    fs_coef lame;        /* vector spaces: FS_COEF_NONE (lame_mu / lame_lambda) or FS_COEF_CELL_LAME; appended last */
} fs_bilinear_form;

/* Replaces dolfin.assemble(a) / the matrix half of assemble_system: numeric
 * cell loop (tabulate_tensor + MatSetValues(ADD)).  add == 0 zeroes A first.  The host arrays of the form have been consumed
 * when the call returns; the cell loop itself is enqueued on the library's stream and the call does NOT wait for it (what the
 * caller does next - the load vector, the Dirichlet rows - is prepared meanwhile; every call that hands data back waits). */
int fs_assemble_matrix(fs_matrix_t A, const fs_bilinear_form* form, int add);

/* Linear form  L(v) = int source * v dx  (body source, ScalarTransportSolver.py:213-226;
 * vector spaces: constant body force f, LinearElasticitySolver.py:227-228, in
 * vector_value) + int div_coef * div v dx (vector spaces only: the thermal-stress load
 * E alpha (T-T0)/(1-2nu) I : grad v, LinearElasticitySolver.py:78-85, 231-238; a nodal
 * coefficient enters by its cell mean, which is what one-point quadrature of a P1 field gives).
 * add == 0 zeroes b first. */
typedef struct fs_linear_form {
    fs_coef source;
    double vector_value[3];
    fs_coef div_coef;
    fs_coef supg_velocity;   /* with supg_pe > 0: + int source * tau (v . grad q) dx (constant, per-cell and nodal sources;
                              * constant / per-cell velocity; nodal: exact for the source's P1 / P2 interpolant) */
    double supg_pe;
} fs_linear_form;
int fs_assemble_vector(fs_space_t space, const fs_linear_form* form, fs_vector_t b, int add);

/* Right-hand side of the L2 projection of the von Mises stress onto the scalar CG1 space of the mesh
 * (LinearElasticitySolver.py:71-76, project(sqrt(3/2 s:s), FunctionSpace(mesh, 'P', 1))): b_a = int vm(u) phi_a dx with
 * s = dev(2 mu sym(grad u) + lambda div u I).  disp_space: 3-vector CG1 or CG2 space, u its dof vector (owned + ghost);
 * p1_space: scalar CG1 space on the SAME mesh.  The projection itself is fs_assemble_matrix(mass = 1) on p1_space +
 * fs_krylov_solve.  CG1 displacement: exact; CG2: 4-point degree-2 rule. */
int fs_assemble_von_mises(fs_space_t disp_space, fs_vector_t u, double mu, double lambda, fs_space_t p1_space, fs_vector_t b);
/* The same with one (mu, lambda) pair per cell: lame[n_cells][2] (host, device cell order). */
int fs_assemble_von_mises_cells(fs_space_t disp_space, fs_vector_t u, const double* lame, fs_space_t p1_space, fs_vector_t b);

/* ---- DG1 advection-diffusion (ScalarTransportDGSolver.py:119-147) -----------------------------------------------------------
 * On a DG matrix: c a(T, v) with the upwind SIPG form
 *   a(T, v) = sum_K int_K (kappa grad v . grad T - T beta . grad v) dx
 *           + sum_F int_F (kappa alpha / h+ [v][T] - kappa {grad v}.n+ [T] - kappa [v] {grad T}.n+ + [v] (b+ T+ - b- T-)) ds
 *           + sum_boundary int_F v max(beta . n, 0) T ds
 * (conductivity = c kappa, h = 2 circumradius, n+ out of the '+' cell, b+- = max(+-beta . n+, 0)), times operator_scale, plus
 * mass_scale int T v dx, plus int h_f T v ds over the listed boundary facets.  b (may be NULL): int source v dx (source: P1 values at
 * every cell's vertices, [n_cells][d+1], device cell order, NULL = none) + int g v ds over the listed facets (facet_g[n_facets][d+1]:
 * the load at the cell's local vertices, the entry of the vertex opposite unused; NULL = none).  Facets: facet_cell[i] (device cell),
 * facet_local[i] (the local vertex opposite), boundary facets only.  One work item per cell writes its own block row: no atomics,
 * two assemblies give the same bits.  add = 0 overwrites A (and b), 1 adds. */
typedef struct fs_dg_form {
    double conductivity;      /* c kappa */
    double capacity;          /* c (multiplies the upwind terms) */
    double velocity[3];       /* beta, constant (2-D: the z component is ignored) */
    double alpha;             /* penalty: 500 in 3-D, 5 in 2-D in the reference */
    double operator_scale;    /* 1 (steady), 1/2 (theta scheme, new step), -1/2 (theta scheme, the old step's right-hand side) */
    double mass_scale;        /* c / dt of the transient term, 0 = none */
    int64_t n_facets;
    const int32_t* facet_cell;
    const int32_t* facet_local;
    const double* facet_h;    /* [n_facets] or NULL */
    const double* facet_g;    /* [n_facets][d+1] or NULL */
    const double* source;     /* [n_cells][d+1] or NULL */
    int add;
} fs_dg_form;
int fs_assemble_dg_transport(fs_matrix_t A, fs_vector_t b, const fs_dg_form* form);
/* Right-hand side of the L2 projection of a DG1 field onto CG1 (ScalarTransportDGSolver.py:194-197): b_i = int T_h phi_i dx, gathered
 * per vertex over its cells in ascending order (no atomics).  V_cg1: scalar CG1 space on the SAME mesh; b has n_vertices entries.
 * The projection is then fs_assemble_matrix(mass = 1) on V_cg1 + fs_krylov_solve. */
int fs_assemble_dg_projection(fs_space_t V_dg, fs_vector_t x, fs_space_t V_cg1, fs_vector_t b);

/* ---- Hyperelasticity (NonlinearElasticitySolver.py:41-98) -------------------------------------------------------------------
 * F = I + grad u, C = F^T F, J = det F, I1 = tr C, I2 = 1/2 (I1^2 - tr C^2), Ibar1 = J^(-2/3) I1, Ibar2 = J^(-4/3) I2.  Energies:
 *   FS_HYPER_NEO_HOOKEAN          psi = mu/2 (I1 - 3) - mu ln J + lambda/2 (ln J)^2                    (the reference's energy)
 *   FS_HYPER_ST_VENANT_KIRCHHOFF  psi = lambda/2 (tr E)^2 + mu E:E,  E = (C - I)/2
 *   FS_HYPER_MOONEY_RIVLIN        psi = c10 (Ibar1 - 3) + c01 (Ibar2 - 3) + kappa/2 (J - 1)^2
 *   FS_HYPER_YEOH                 psi = c10 (Ibar1 - 3) + c20 (Ibar1 - 3)^2 + c30 (Ibar1 - 3)^3 + kappa/2 (J - 1)^2
 * The last three have no counterpart in the reference.  Parameters: neo-Hookean and St Venant-Kirchhoff take mu / lambda (or the
 * per-cell pairs of `lame`); Mooney-Rivlin takes params = (c10, c01, kappa, -) and Yeoh params = (c10, c20, c30, kappa), or one such
 * row per cell in `cell_params`.
 * 2-D is plane strain.  For the three new energies F is the 3 x 3 matrix with the in-plane 2 x 2 block and F33 = 1, the invariants are
 * the 3-D ones and psi = 0 at u = 0.  The 2-D neo-Hookean energy keeps the reference's form: F is 2 x 2 and the "- 3" stays, which
 * shifts the energy by -mu/2 per unit area and changes nothing else.
 * fs_assemble_hyperelastic evaluates at the displacement u, on a vector CG1 space over tetrahedra or triangles (one rank):
 *   FS_HYPER_TANGENT  K = d^2 Pi / du^2, the tangent stiffness (pattern of the space, no Dirichlet rows);
 *   FS_HYPER_FORCE    r = d Pi / du, the internal force int P : grad v dx (owned dofs);
 *   FS_HYPER_ENERGY   info->energy = int psi dx.
 * External loads do not depend on u: they are assembled with fs_assemble_vector / fs_assemble_facet_vector.
 * u: dof vector (node-interleaved, >= n_dofs_local entries).  K and r are overwritten, or added to with form->add.  Every result is
 * deterministic (no atomics; the energy is summed in a fixed order).  At u = 0 the neo-Hookean tangent equals fs_assemble_matrix of
 * the linear elasticity operator with the same (mu, lambda) bit for bit; the tangent of the other energies equals the operator of
 * their small-strain moduli (mu0 = mu, 2 (c10 + c01), 2 c10; lambda0 = lambda, kappa - 2 mu0 / 3) to rounding.
 * info (optional unless FS_HYPER_ENERGY): the energy, the number of cells with J <= 0 or J not finite (where the tangent, the force
 * and the energy are meaningless) and one of them, in the caller's cell numbering (-1: none).  info is filled whatever `what`
 * holds.
 * Refused with FS_ERR_INVALID and a message (naming the cell, in device order, for per-cell data): other spaces, several ranks, an
 * unknown model, any parameter that is not finite, and
 *   neo-Hookean, St Venant-Kirchhoff: mu <= 0 or lambda < 0;
 *   Mooney-Rivlin: c10 < 0, c01 < 0, c10 + c01 <= 0 or kappa <= 0;
 *   Yeoh: c10 <= 0 or kappa <= 0 (c20 and c30 may have either sign: fitted c20 are usually negative).
 * St Venant-Kirchhoff loses ellipticity under strong compression; nothing here guards against that.
 *
 * fs_hyper_stress: the Cauchy stress sigma = P F^T / J per cell for all four energies, into the HOST array sigma[n_cells][6] =
 * (xx, yy, zz, xy, xz, yz), in plane strain sigma[n_cells][4] = (xx, yy, zz, xy) with sigma_zz kept - tensor components, cells in
 * device cell order, as fs_anisotropic_stress.  `add` is ignored.  A state with an inverted cell is refused (FS_ERR_INVALID, the
 * message names the count and the first cell in the caller's numbering; info, if given, holds them) and sigma is left untouched. */
#define FS_HYPER_NEO_HOOKEAN 0
#define FS_HYPER_ST_VENANT_KIRCHHOFF 1
#define FS_HYPER_MOONEY_RIVLIN 2
#define FS_HYPER_YEOH 3
#define FS_HYPER_TANGENT 1
#define FS_HYPER_FORCE 2
#define FS_HYPER_ENERGY 4
#define FS_COEF_CELL_HYPER 11 /* fs_hyper_form.cell_params only: data[n_cells][4], one parameter row per cell in device cell order */
typedef struct fs_hyper_form {
    int model;           /* FS_HYPER_NEO_HOOKEAN, _ST_VENANT_KIRCHHOFF, _MOONEY_RIVLIN or _YEOH */
    double mu, lambda;   /* neo-Hookean, St Venant-Kirchhoff: Lame parameters when lame.mode == FS_COEF_NONE */
    fs_coef lame;        /* FS_COEF_NONE or FS_COEF_CELL_LAME: data[n_cells][2] = (mu, lambda), host, device cell order */
    int add;             /* 0: overwrite K / r; 1: add to them */
    double params[4];    /* Mooney-Rivlin (c10, c01, kappa, -), Yeoh (c10, c20, c30, kappa) when cell_params.mode == FS_COEF_NONE */
    fs_coef cell_params; /* FS_COEF_NONE or FS_COEF_CELL_HYPER: data[n_cells][4], rows as params, host, device cell order */
} fs_hyper_form;
typedef struct fs_hyper_info {
    double energy;
    int64_t n_inverted;
    int64_t first_inverted_cell;
} fs_hyper_info;
int fs_assemble_hyperelastic(fs_space_t space, fs_matrix_t K, fs_vector_t r, fs_vector_t u, const fs_hyper_form* form, int what,
                             fs_hyper_info* info);
int fs_hyper_stress(fs_space_t space, fs_vector_t u, const fs_hyper_form* form, double* sigma, fs_hyper_info* info);

/* ---- Small-strain J2 plasticity (PlasticitySolver; the reference names the class in its Readme and never delivers it) ----------
 * Rate-independent von Mises plasticity with linear isotropic hardening on a vector CG1 space over tetrahedra or triangles (plane
 * strain), one rank.  One integration point per cell: eps = sym grad u, e = eps - eps_p,
 *   sigma_tr = K tr(e) I + 2 G dev(e),  s = dev sigma_tr,  q = sqrt(3/2) |s|,  f = q - (yield_stress + hardening * p);
 *   f <= 0: sigma = sigma_tr, D = C, history unchanged;
 *   f >  0: dp = f / (3 G + hardening), N = s / |s|, beta = 3 G dp / q, sigma = sigma_tr - 2 G dp sqrt(3/2) N,
 *           eps_p += sqrt(3/2) dp N, p += dp, D = C - 2 G beta I_dev - 2 G (3G / (3G + hardening) - beta) N (x) N.
 * The history object holds, per cell in DEVICE cell order, the committed state (eps_p, p, returned stress) and the trial state of
 * the last fs_assemble_plasticity.  Tensors are stored as (xx, yy, zz, xy, xz, yz) in 3-D and (xx, yy, zz, xy) in plane strain
 * (eps_zz = 0, but eps_p,zz and sigma_zz are not): n_comp = 6 or 4 tensor components per cell.
 *   fs_plastic_state_create   a history on the space, all zero          fs_plastic_state_destroy  frees it
 *   fs_plastic_state_reset    committed and trial state back to zero    fs_plastic_state_commit   trial -> committed (a converged step)
 *   fs_plastic_state_get      which = FS_PLASTIC_COMMITTED / FS_PLASTIC_TRIAL: eps_p[n_cells][n_comp], p[n_cells],
 *                             stress[n_cells][n_comp] to the host (any of the three may be NULL)
 *   fs_plastic_state_set      the committed eps_p and p from the host (p >= 0 in every cell)
 * fs_assemble_plasticity evaluates at the displacement u from the COMMITTED history, which it does not change:
 *   FS_PLASTIC_TANGENT  K = int B^T D B dx, the consistent tangent (pattern of the space, no Dirichlet rows);
 *   FS_PLASTIC_FORCE    r = int sigma : grad v dx, the internal force of the returned stress (owned dofs).
 * The return mapping runs once per cell and writes the trial state; tangent and force are gathered from it without atomics, so a
 * repeated call gives the same bits.  While no cell yields, the tangent equals fs_assemble_matrix of the linear elasticity operator
 * with the same (mu, lambda) bit for bit.  K and r are overwritten, or added to with form->add.
 * info (optional): the cells with f > 0 in this evaluation, the cells whose f is not finite (their results are meaningless) and one
 * of those in the caller's cell numbering (-1: none).  Other spaces, several ranks, a history of another space, mu <= 0, lambda < 0,
 * yield_stress <= 0 or hardening < 0 (constant or in any cell): FS_ERR_INVALID with a message. */
#define FS_COEF_CELL_PLASTIC 9 /* fs_plastic_form.material only: data[n_cells][4] = (mu, lambda, yield_stress, hardening) per cell */
#define FS_PLASTIC_TANGENT 1
#define FS_PLASTIC_FORCE 2
#define FS_PLASTIC_COMMITTED 0
#define FS_PLASTIC_TRIAL 1
typedef struct fs_plastic_state_s* fs_plastic_state_t;
typedef struct fs_plastic_form {
    double mu, lambda;              /* Lame parameters (G = mu) when material.mode == FS_COEF_NONE */
    double yield_stress, hardening; /* sigma_y > 0 and H = d sigma_y / dp >= 0, likewise */
    fs_coef material;               /* FS_COEF_NONE or FS_COEF_CELL_PLASTIC (host, device cell order) */
    int add;                        /* 0: overwrite K / r; 1: add to them */
} fs_plastic_form;
typedef struct fs_plastic_info {
    int64_t n_yielded;
    int64_t n_nonfinite;
    int64_t first_nonfinite_cell;
} fs_plastic_info;
int fs_plastic_state_create(fs_space_t space, fs_plastic_state_t* out);
int fs_plastic_state_destroy(fs_plastic_state_t state);
int fs_plastic_state_reset(fs_plastic_state_t state);
int fs_plastic_state_commit(fs_plastic_state_t state);
int fs_plastic_state_get(fs_plastic_state_t state, int which, double* eps_p, double* p, double* stress);
int fs_plastic_state_set(fs_plastic_state_t state, const double* eps_p, const double* p);
int fs_assemble_plasticity(fs_space_t space, fs_matrix_t K, fs_vector_t r, fs_vector_t u, fs_plastic_state_t state,
                           const fs_plastic_form* form, int what, fs_plastic_info* info);

/* ---- Small-strain linear viscoelasticity (ViscoelasticitySolver; the reference lists "viscoelastic" in its Readme and has none) ----
 * Generalized Maxwell solid (Prony series) on a vector CG1 space over tetrahedra or triangles (plane strain), one rank, one
 * integration point per cell.  Elastic bulk response, relaxing deviatoric response; with e = dev eps:
 *   sigma(t) = K tr(eps) I + 2 G0 [ g_inf e + sum_k g_k h_k ],  h_k(t) = int_0^t exp(-(t - s) / tau_k) de/ds ds,  g_inf = 1 - sum_k g_k,
 * G0 = mu and K = lambda + 2/3 mu the INSTANTANEOUS moduli.  One step of length dt (exact for a strain linear within the step), with
 * x_k = dt / tau_k:  a_k = exp(-x_k),  b_k = -expm1(-x_k) / x_k  (for x_k < 1e-5 the series 1 - x/2 + x^2/6 - x^3/24, which agrees
 * with the quotient to rounding there and has the limit 1 at x = 0),  h_k^{n+1} = a_k h_k^n + b_k (e^{n+1} - e^n).
 * A step is one linear solve  K(mu_eff, lambda_eff) u^{n+1} = f_ext - int B^T s_hist dx  with the operator of fs_assemble_matrix and
 *   mu_eff = G0 (g_inf + sum_k g_k b_k),  lambda_eff = K - 2/3 mu_eff,  s_hist = 2 G0 sum_k g_k (a_k h_k^n - b_k e^n).
 * The history object holds, per cell in DEVICE cell order, the committed state (e, h_k, stress) and the trial state of the last
 * update.  Tensors are stored as (xx, yy, zz, xy, xz, yz) in 3-D and (xx, yy, zz, xy) in plane strain (eps_zz = 0, but e_zz, h_k,zz and
 * sigma_zz are not): n_comp = 6 or 4 tensor components; h is [n_cells][n_terms][n_comp].
 *   fs_visco_state_create   a history for n_terms Prony terms (0 .. FS_VISCO_MAX_TERMS), all zero     fs_visco_state_destroy  frees it
 *   fs_visco_state_reset    committed and trial state back to zero    fs_visco_state_commit   trial -> committed (a converged step)
 *   fs_visco_state_get      which = FS_VISCO_COMMITTED / FS_VISCO_TRIAL: e[n_cells][n_comp], h[n_cells][n_terms][n_comp],
 *                           stress[n_cells][n_comp] to the host (any of the three may be NULL)
 *   fs_visco_state_set      the committed e and h from the host (finite values; h may be NULL when n_terms = 0)
 * fs_assemble_viscoelastic does, in this order, what the bits of `what` ask for; it never changes the committed state:
 *   FS_VISCO_LOAD    r = -int B^T s_hist dx from the COMMITTED (e, h_k) and this step's (a_k, b_k) (owned dofs; u may be NULL);
 *   FS_VISCO_UPDATE  the trial state (e, h_k, sigma) at the displacement u from the committed one (r may be NULL);
 *   FS_VISCO_FORCE   r = int B^T sigma dx of the TRIAL stress (not together with FS_VISCO_LOAD: both write r).
 * The update runs once per cell; r is gathered per node over the cells around it in ascending order, without atomics: a repeated
 * call gives the same bits, and a per-cell material that holds one constant gives the bits of that constant.  r is overwritten, or
 * added to with form->add.  info (optional): the cells whose updated stress is not finite, one of them in the caller's cell
 * numbering (-1: none), and the device time of each pass.  FS_ERR_INVALID with a message (which names the cell, in device order, for a per-cell material): other spaces,
 * several ranks, a history of another space or another n_terms, n_terms > FS_VISCO_MAX_TERMS, mu <= 0, lambda + 2/3 mu <= 0,
 * g_k <= 0, tau_k <= 0, sum g_k >= 1, dt <= 0 or not finite. */
#define FS_VISCO_MAX_TERMS 8
#define FS_COEF_CELL_VISCO 10 /* fs_visco_form.material only: data[n_cells][2 + 2 n_terms] = (mu, lambda, g_1, tau_1, g_2, tau_2, ...) per cell */
#define FS_VISCO_LOAD 1
#define FS_VISCO_UPDATE 2
#define FS_VISCO_FORCE 4
#define FS_VISCO_COMMITTED 0
#define FS_VISCO_TRIAL 1
typedef struct fs_visco_state_s* fs_visco_state_t;
typedef struct fs_visco_form {
    double mu, lambda;              /* instantaneous Lame parameters (G0 = mu) when material.mode == FS_COEF_NONE */
    int n_terms;                    /* Prony terms, 0 (elastic) .. FS_VISCO_MAX_TERMS; the history's n_terms */
    double g[FS_VISCO_MAX_TERMS];   /* relative moduli g_k > 0, sum < 1, when material.mode == FS_COEF_NONE */
    double tau[FS_VISCO_MAX_TERMS]; /* relaxation times tau_k > 0, likewise */
    fs_coef material;               /* FS_COEF_NONE or FS_COEF_CELL_VISCO (host, device cell order) */
    double dt;                      /* the step length, > 0 */
    int add;                        /* 0: overwrite r; 1: add to it */
} fs_visco_form;
typedef struct fs_visco_info {
    int64_t n_nonfinite;
    int64_t first_nonfinite_cell;
    double load_ms, update_ms, force_ms; /* HIP-event time of the passes this call ran (0: not run); load and update include the
                                            launch that tabulates (a_k, b_k) for a constant material */
} fs_visco_info;
int fs_visco_state_create(fs_space_t space, int n_terms, fs_visco_state_t* out);
int fs_visco_state_destroy(fs_visco_state_t state);
int fs_visco_state_reset(fs_visco_state_t state);
int fs_visco_state_commit(fs_visco_state_t state);
int fs_visco_state_get(fs_visco_state_t state, int which, double* e, double* h, double* stress);
int fs_visco_state_set(fs_visco_state_t state, const double* e, const double* h);
int fs_assemble_viscoelastic(fs_space_t space, fs_vector_t r, fs_vector_t u, fs_visco_state_t state, const fs_visco_form* form, int what,
                             fs_visco_info* info);

/* ---- Explicit scalar wave propagation (WaveSolver; the reference lists "wave propagation" in its Readme and has none) --------
 * u_tt = div(c^2 grad u) + f on a scalar CG1 space over tetrahedra or triangles, one rank: central differences with a lumped mass,
 * so a step is ONE product with the assembled stiffness K (coefficient c^2, fs_assemble_matrix) and one pointwise update - no solve.
 * Per row i: m_i = int phi_i dx (lumped mass, > 0), d_i >= 0 (lumped first-order absorbing boundary: the sum over the absorbing
 * facets F around i of c |F| / dim), F_i the load; every load shares one time factor, f^n = s_f[n] F, and Dirichlet rows take
 * g_i s_g[n].  Step n -> n+1 (n >= 1), with y = K u^n:
 *   (m/dt^2 + d/(2 dt)) u^{n+1} = s_f[n] F - y + (2 m/dt^2) u^n - (m/dt^2 - d/(2 dt)) u^{n-1},  then u^{n+1}_i = g_i s_g[n+1] on Dirichlet rows.
 * Start: a^0 = (s_f[0] F - K u^0 - d v^0) / m,  u^1 = u^0 + dt v^0 + dt^2/2 a^0 (Dirichlet rows: g s_g[1]).
 * Discrete energy of step n -> n+1, its two halves reported separately:
 *   E_kin = 1/2 sum_i m_i ((u^{n+1} - u^n)_i / dt)^2,   E_pot = 1/2 (u^{n+1})^T y   (constant for d = 0, F = 0 and fixed Dirichlet values).
 * The state object holds u^{n-1}, u^n and a work field (rotated by pointer), the device copies of m, d, F, the Dirichlet rows and
 * their values (uploaded once by fs_wave_state_configure; a Dirichlet row keeps g_i in the slot of F_i) and the step counter n.
 *   fs_wave_state_create     a zero state (n = 0) on a scalar CG1 space             fs_wave_state_destroy   frees it
 *   fs_wave_state_configure  dt and the arrays mass[n_dofs], damping[n_dofs] (NULL: none), load[n_dofs] (NULL: none), the Dirichlet
 *                            dofs and values (a dof named twice takes the last value)
 *   fs_wave_state_set / get  (u^{n-1}, u^n) and the step counter n from / to the host (get: any pointer may be NULL)
 *   fs_wave_start            forms u^1 from (u^0, v^0) with s_f[0] and s_g[1]: the state then holds (u^0, u^1), n = 1
 * fs_wave_advance enqueues n_steps steps on the library's stream with no host synchronisation between them: per step the product
 * of K through the dispatch of fs_spmv, then ONE update kernel over the rows (the formula, the Dirichlet rows, the per-workgroup
 * partials of both energy halves, the receiver samples).  Step k of the call advances n -> n+1 with load_scale[k] = s_f[n] and
 * dirichlet_scale[k] = s_g[n+1]; traces[k][r] = u^{n+1}[receiver_dofs[r]] and energy[k] = (E_kin, E_pot) of that step (either may
 * be NULL).  The partials are summed in a fixed order by a finishing pass (no floating-point atomics): a repeated run gives the
 * same bits, and so does any split of a march into calls.  A non-finite field value makes the energy of its step non-finite: the
 * finishing pass counts those steps on the device, read once per call.  The call waits for the device only if it hands data back
 * (traces, energy or info).  FS_ERR_INVALID with a message: spaces other than scalar CG1, several ranks, a matrix of another space,
 * dt <= 0 or not finite, m_i <= 0, d_i < 0, a receiver or Dirichlet dof out of range, a state that was not configured / started. */
typedef struct fs_wave_state_s* fs_wave_state_t;
typedef struct fs_march_info {    /* what a batch of explicit steps reports (fs_wave_advance, fs_dyn_explicit_advance) */
    double device_ms;             /* HIP-event time of the whole batch (products, updates, finishing passes) */
    int64_t n_nonfinite;          /* steps of this call whose energy (hence: field) is not finite */
    int64_t first_nonfinite_step; /* the first of them, as its index k in this call; -1: none */
    int64_t step;                 /* the state's step counter n after the call */
} fs_march_info;
typedef fs_march_info fs_wave_info;
int fs_wave_state_create(fs_space_t space, fs_wave_state_t* out);
int fs_wave_state_destroy(fs_wave_state_t state);
int fs_wave_state_configure(fs_wave_state_t state, double dt, const double* mass, const double* damping, const double* load,
                            int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values);
int fs_wave_state_set(fs_wave_state_t state, const double* u_prev, const double* u, int64_t step);
int fs_wave_state_get(fs_wave_state_t state, double* u_prev, double* u, int64_t* step);
int fs_wave_start(fs_matrix_t K, fs_wave_state_t state, const double* u0, const double* v0, double load_scale0, double dirichlet_scale1);
int fs_wave_advance(fs_matrix_t K, fs_wave_state_t state, int64_t n_steps, const double* load_scale, const double* dirichlet_scale,
                    int64_t n_receivers, const int32_t* receiver_dofs, double* traces, double* energy, fs_wave_info* info);

/* ---- Implicit structural dynamics (ElastodynamicsSolver; the reference has no transient structural solver) --------------------
 * M a + C v + K u = s_f(t) F on a vector CG1 or CG2 space over tetrahedra or triangles (plane strain), one rank: K the isotropic
 * elasticity operator, M the consistent mass, C = eta_M M + eta_K K, marched by the Chung-Hulbert generalized-alpha scheme.  With
 * x_{n+1-alpha} = (1 - alpha) x_{n+1} + alpha x_n the balance of a step is
 *   M a_{n+1-am} + C v_{n+1-af} + K u_{n+1-af} = s_f(t_n + (1 - af) dt) F,
 *   u~ = u_n + dt v_n + dt^2 (1/2 - beta) a_n,   v~ = v_n + dt (1 - gamma) a_n,
 *   a_{n+1} = (u_{n+1} - u~) / (beta dt^2),       v_{n+1} = v~ + gamma dt a_{n+1}.
 * Solved for u_{n+1} a step is ONE linear solve with the fixed operator
 *   K_eff = c_M M + c_K K,   c_M = (1 - am)/(beta dt^2) + (1 - af) gamma eta_M/(beta dt),   c_K = (1 - af)(1 + gamma eta_K/(beta dt)),
 *   cv  = (1 - af)(v~ - gamma/(beta dt) u~) + af v_n,
 *   p   = (1 - am) u~/(beta dt^2) - am a_n - eta_M cv - c_M g_ext,      q = -af u_n - eta_K cv - c_K g_ext,
 *   rhs = s_f F + M p + K q on the free rows,   rhs_i = g_i s_g(t_{n+1}) on the Dirichlet rows;
 * g_ext = the next Dirichlet values on the Dirichlet dofs, zero elsewhere (its two terms are the lifting of the Dirichlet columns).
 * K and M are the operators WITHOUT eliminated rows.  K_eff, with its Dirichlet rows and columns eliminated, is the caller's: built
 * once per step length and solved with (fs_amg_solve / fs_krylov_solve) between fs_dyn_predict and fs_dyn_correct.
 * The state object holds u, v, a, the work vectors p, q, M p, K q, the load F (a Dirichlet row keeps g_i in the slot of F_i), one
 * flag byte per row (Dirichlet bit, receiver bit), the constants of the scheme and the step counter n (-1: not started).
 *   fs_dyn_state_create      a zero state on a vector CG space                      fs_dyn_state_destroy   frees it
 *   fs_dyn_state_configure   dt, (alpha_m, alpha_f, beta, gamma), eta_M, eta_K, load[n_dofs] (NULL: none), the Dirichlet dofs and
 *                            values (a dof named twice takes the last value); keeps (u, v, a) and the step counter
 *   fs_dyn_state_set / get   (u, v, a) and the step counter from / to the host (get: any pointer may be NULL)
 *   fs_dyn_state_get_work    p, q, M p, K q of the last fs_dyn_predict to the host (any pointer may be NULL): for checks
 *   fs_dyn_state_info        waits for the device: the times of the last predict / correct, the non-finite rows seen since the start
 *   fs_dyn_start_rhs         takes (u_0, v_0) and forms rhs = s_f(t_0) F - C v_0 - K u_0 on the free rows, 0 on the Dirichlet rows;
 *   fs_dyn_start             takes a_0, solved by the caller from that right-hand side with the eliminated M (a_0 = 0 on Dirichlet
 *                            rows): the state then holds (u_0, v_0, a_0), n = 0
 *   fs_dyn_predict           one kernel forms p and q, two products through the dispatch of fs_spmv, one kernel forms rhs; nothing
 *                            returns to the host.  load_scale = s_f(t_n + (1 - af) dt), dirichlet_scale_next = s_g(t_{n+1})
 *   fs_dyn_correct           x = u_{n+1}: one kernel forms a_{n+1}, v_{n+1}, takes u_{n+1} in place (Dirichlet rows by the same
 *                            formulas), writes the receiver samples of u_{n+1} and counts non-finite rows; n -> n+1.  It waits for
 *                            the device only when samples is not NULL (samples[n_receivers])
 *   fs_dyn_energy            out = (1/2 v^T M v, 1/2 u^T K u): two products, per-workgroup partials summed in a fixed order
 * No floating-point atomics: a march gives the same bits however it is split into calls.  FS_ERR_INVALID with a message: scalar or
 * DG spaces, several ranks, matrices of another space, dt <= 0 or not finite, parameters outside alpha_m <= alpha_f <= 1/2,
 * beta >= 1/4 + (alpha_f - alpha_m)/2 (not unconditionally stable), eta < 0, a receiver or Dirichlet dof out of range, a state that was
 * not configured / started; a refused call leaves the state as it was. */
typedef struct fs_dyn_state_s* fs_dyn_state_t;
typedef struct fs_dyn_info {
    double predict_ms;            /* HIP-event time of the last fs_dyn_predict (both kernels and both products) */
    double predict_pointwise_ms;  /* ... of its two kernels alone */
    double correct_ms;            /* ... of the kernel of the last fs_dyn_correct */
    int64_t n_nonfinite;          /* rows found non-finite by fs_dyn_correct since the start */
    int64_t first_nonfinite_step; /* the first step n+1 that had one; -1: none */
    int64_t step;                 /* the state's step counter n */
} fs_dyn_info;
int fs_dyn_state_create(fs_space_t space, fs_dyn_state_t* out);
int fs_dyn_state_destroy(fs_dyn_state_t state);
int fs_dyn_state_configure(fs_dyn_state_t state, double dt, double alpha_m, double alpha_f, double beta, double gamma, double eta_m,
                           double eta_k, const double* load, int64_t n_dirichlet, const int32_t* dirichlet_dofs,
                           const double* dirichlet_values);
int fs_dyn_state_set(fs_dyn_state_t state, const double* u, const double* v, const double* a, int64_t step);
int fs_dyn_state_get(fs_dyn_state_t state, double* u, double* v, double* a, int64_t* step);
int fs_dyn_state_get_work(fs_dyn_state_t state, double* p, double* q, double* mp, double* kq);
int fs_dyn_state_info(fs_dyn_state_t state, fs_dyn_info* info);
int fs_dyn_start_rhs(fs_matrix_t K, fs_matrix_t M, fs_dyn_state_t state, const double* u0, const double* v0, double load_scale0,
                     fs_vector_t rhs);
int fs_dyn_start(fs_dyn_state_t state, fs_vector_t a0);
int fs_dyn_predict(fs_matrix_t K, fs_matrix_t M, fs_dyn_state_t state, double load_scale, double dirichlet_scale_next, fs_vector_t rhs);
int fs_dyn_correct(fs_dyn_state_t state, fs_vector_t x, int64_t n_receivers, const int32_t* receiver_dofs, double* samples);
int fs_dyn_energy(fs_matrix_t K, fs_matrix_t M, fs_dyn_state_t state, double* out);

/* ---- Explicit structural dynamics (ElastodynamicsSolver, 'scheme': 'explicit') --------------------------------------------------
 * M a + C v + K u = s_f(t) F on a vector CG1 space over tetrahedra or triangles (plane strain), one rank: central differences with
 * the lumped mass m = M 1 (the row sums of the consistent mass, > 0 on CG1) and mass-proportional damping C = eta_M diag(m), so a
 * step is ONE product with the elasticity operator K (WITHOUT eliminated rows) and one pointwise update - no solve.  The state is
 * (u_n, w_n) with w_n = v_{n-1/2}; with y_n = K u_n and alpha = eta_M dt / 2 a step n -> n+1 (n >= 1) is, per row i,
 *   (1 + alpha) w_{n+1/2} = (1 - alpha) w_{n-1/2} + dt (s_f[n] F - y_n) / m,      u_{n+1} = u_n + dt w_{n+1/2},
 * and on a Dirichlet row u_{n+1} = g_i s_g[n+1], w_{n+1/2} = (u_{n+1} - u_n) / dt.
 * Start: the Dirichlet rows of u_0 take g s_g[0]; a_0 = (s_f[0] F - y_0) / m - eta_M v_0, w_{1/2} = v_0 + dt/2 a_0, u_1 = u_0 +
 * dt w_{1/2} (Dirichlet rows by the rule above, with s_g[1]).
 * Discrete energy of step n -> n+1, its two halves reported separately:
 *   E_kin = 1/2 sum_i m_i w_{n+1/2,i}^2,   E_pot = 1/2 u_{n+1}^T y_n;
 * with F = 0 and fixed Dirichlet values E_{n+1/2} - E_{n-1/2} = -eta_M dt v_n^T diag(m) v_n exactly (constant for eta_M = 0).
 * The state object holds u and w (updated in place), the last product y, the device copies of m, F, the Dirichlet rows and their
 * values (a Dirichlet row keeps g_i in the slot of F_i), one flag byte per row and the step counter n (0: not started).
 *   fs_dyn_explicit_state_create     a zero state (n = 0) on a vector CG1 space     fs_dyn_explicit_state_destroy   frees it
 *   fs_dyn_explicit_state_configure  dt, eta_M and the arrays mass[n_dofs], load[n_dofs] (NULL: none), the Dirichlet dofs and values
 *                                    (a dof named twice takes the last value); keeps (u, w) and the step counter
 *   fs_dyn_explicit_state_set / get  (u_n, w_n) and the step counter n >= 1 from / to the host (get: any pointer may be NULL)
 *   fs_dyn_explicit_state_get_work   the last y to the host: for checks
 *   fs_dyn_explicit_start            forms (u_1, w_{1/2}) from (u_0, v_0) with s_f[0], s_g[0] and s_g[1]: n = 1
 *   fs_dyn_explicit_full_step        v_n = (w_{n-1/2} + w+)/2 and a_n = (w+ - w_{n-1/2})/dt of the state's time point, with w+ the
 *                                    recurrence's w_{n+1/2} under load_scale_n = s_f[n] (one product; w+ is not stored and the state
 *                                    does not change); on Dirichlet rows v_n = w_{n-1/2}, a_n = 0.  Either output may be NULL
 * fs_dyn_explicit_advance enqueues n_steps steps on the library's stream with no host synchronisation between them: per step the
 * product of K through the dispatch of fs_spmv, then ONE update kernel over the rows (the formula, the Dirichlet rows, the
 * per-workgroup partials of both energy halves, the receiver samples; 57 B per row).  Step k of the call advances n -> n+1 with
 * load_scale[k] = s_f[n] and dirichlet_scale[k] = s_g[n+1]; traces[k][r] = u_{n+1}[receiver_dofs[r]] and energy[k] = (E_kin, E_pot)
 * of that step (either may be NULL).  The partials are summed in a fixed order by a finishing pass (no floating-point atomics): a
 * repeated run gives the same bits, and so does any split of a march into calls.  A non-finite field value makes the energy of
 * its step or of the next one non-finite: the finishing pass counts those steps on the device, read once per call.  The call
 * waits for the device only if it hands data back (traces, energy or info).  FS_ERR_INVALID with a message: spaces other than
 * vector CG1, several ranks, a matrix of another space, dt <= 0 or not finite, eta_M < 0, m_i <= 0, a time factor that is not
 * finite, a receiver or Dirichlet dof out of range, a state that was not configured / started; a refused call leaves the state as
 * it was. */
typedef struct fs_dyn_explicit_state_s* fs_dyn_explicit_state_t;
typedef fs_march_info fs_dyn_explicit_info;
int fs_dyn_explicit_state_create(fs_space_t space, fs_dyn_explicit_state_t* out);
int fs_dyn_explicit_state_destroy(fs_dyn_explicit_state_t state);
int fs_dyn_explicit_state_configure(fs_dyn_explicit_state_t state, double dt, double eta_m, const double* mass, const double* load,
                                    int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values);
int fs_dyn_explicit_state_set(fs_dyn_explicit_state_t state, const double* u, const double* w, int64_t step);
int fs_dyn_explicit_state_get(fs_dyn_explicit_state_t state, double* u, double* w, int64_t* step);
int fs_dyn_explicit_state_get_work(fs_dyn_explicit_state_t state, double* y);
int fs_dyn_explicit_start(fs_matrix_t K, fs_dyn_explicit_state_t state, const double* u0, const double* v0, double load_scale0,
                          double dirichlet_scale0, double dirichlet_scale1);
int fs_dyn_explicit_advance(fs_matrix_t K, fs_dyn_explicit_state_t state, int64_t n_steps, const double* load_scale,
                            const double* dirichlet_scale, int64_t n_receivers, const int32_t* receiver_dofs, double* traces,
                            double* energy, fs_dyn_explicit_info* info);
int fs_dyn_explicit_full_step(fs_matrix_t K, fs_dyn_explicit_state_t state, double load_scale_n, double* v_out, double* a_out);

/* ---- Explicit finite-strain dynamics (HyperelasticDynamicsSolver; no counterpart in the reference) ------------------------------
 * M a + C v + f_int(u) = s_f(t) F on a vector CG1 space over tetrahedra or triangles (true plane strain), one rank: the scheme of
 * fs_dyn_explicit_* with the product K u_n replaced by the internal force f_int(u_n) = dPi/du of one of the four energies of
 * fs_hyper_form, evaluated at the current displacement in every step.  Lumped mass m = M 1 of the reference configuration,
 * C = eta_M diag(m), alpha = eta_M dt / 2; the state is (u_n, w_n) with w_n = v_{n-1/2} and a step n -> n+1 (n >= 1) is, per row i,
 *   (1 + alpha) w_{n+1/2} = (1 - alpha) w_{n-1/2} + dt (s_f[n] F - f_int(u_n)) / m,      u_{n+1} = u_n + dt w_{n+1/2},
 * and on a Dirichlet row u_{n+1} = g_i s_g[n+1], w_{n+1/2} = (u_{n+1} - u_n) / dt.  Start: the Dirichlet rows of u_0 take g s_g[0];
 * a_0 = (s_f[0] F - f_int(u_0)) / m - eta_M v_0, w_{1/2} = v_0 + dt/2 a_0, u_1 = u_0 + dt w_{1/2} (Dirichlet rows by the rule above,
 * with s_g[1]).  Loads are dead loads.  Energy of the step n -> n+1, its two halves reported separately:
 *   E_kin = 1/2 sum_i m_i w_{n+1/2,i}^2,   Pi(u_n) = int psi(F(u_n)) dx
 * - the potential half is taken at t_n, where the force is evaluated (fs_dyn_explicit_advance reports 1/2 u_{n+1}^T K u_n).  psi = 0
 * at rest for all four energies in both dimensions: in plane strain the neo-Hookean energy is taken with F embedded in 3 x 3 like
 * the other three (the "- 3" shift of the 2-D energy of fs_assemble_hyperelastic does not appear here).
 * A step is ONE kernel launch: one thread per node gathers the force and its share of Pi over the incident cells and applies the
 * update, the Dirichlet rows, the receiver samples and the energy partials.  u is double-buffered inside the state (the gather reads
 * the neighbours' u_n while their threads write u_{n+1}); the buffers swap per step and the calls below always see u_n.
 *   fs_hyper_dyn_state_create     a zero state (n = 0) on a vector CG1 space     fs_hyper_dyn_state_destroy   frees it
 *   fs_hyper_dyn_state_configure  dt, eta_M and the arrays mass[n_dofs], load[n_dofs] (NULL: none), the Dirichlet dofs and values
 *                                 (a dof named twice takes the last value); keeps (u, w) and the step counter
 *   fs_hyper_dyn_state_set / get  (u_n, w_n) and the step counter n >= 1 from / to the host (get: any pointer may be NULL)
 *   fs_hyper_dyn_start            forms (u_1, w_{1/2}) from (u_0, v_0) with s_f[0], s_g[0] and s_g[1]: n = 1
 *   fs_hyper_dyn_advance          n_steps steps enqueued back to back with no host synchronisation between them; step k of the call
 *                                 advances n -> n+1 with load_scale[k] = s_f[n] and dirichlet_scale[k] = s_g[n+1];
 *                                 traces[k][r] = u_{n+1}[receiver_dofs[r]], energy[k] = (E_kin(w_{n+1/2}), Pi(u_n)) (either may be NULL)
 *   fs_hyper_dyn_full_step        v_n = (w_{n-1/2} + w+)/2 and a_n = (w+ - w_{n-1/2})/dt of the state's time point, w+ the recurrence's
 *                                 w_{n+1/2} under load_scale_n = s_f[n] (the force is recomputed, nothing is stored, the state does
 *                                 not change); on Dirichlet rows v_n = w_{n-1/2}, a_n = 0.  Either output may be NULL
 *   fs_hyper_dyn_internal_force   f_int(u_n)[n_dofs] and Pi(u_n) of the held state (either may be NULL)
 * form: the material, constant parameters or per-cell rows as for fs_assemble_hyperelastic (`add` is ignored); it is checked at every
 * call and uploaded only when it differs from what the state holds - never per step.
 * A cell with J <= 0 or J not finite makes Pi of its step NaN (for every energy: St Venant-Kirchhoff itself stays finite there), so
 * the finishing pass of the batch counts that step in info->n_nonfinite / first_nonfinite_step, as it counts a non-finite field.
 * The energy partials are summed in a fixed order (no floating-point atomics): a repeated run gives the same bits, and so does any
 * split of a march into calls.  The call waits for the device only if it hands data back (traces, energy or info).
 * FS_ERR_INVALID with a message: DG, CG2 or scalar spaces, several ranks, dt <= 0 or not finite, eta_M < 0, m_i <= 0, an unknown
 * model or a parameter row its model refuses (fs_assemble_hyperelastic), a time factor that is not finite, a receiver or Dirichlet
 * dof out of range, a state that was not configured / started. */
typedef struct fs_hyper_dyn_state_s* fs_hyper_dyn_state_t;
int fs_hyper_dyn_state_create(fs_space_t space, fs_hyper_dyn_state_t* out);
int fs_hyper_dyn_state_destroy(fs_hyper_dyn_state_t state);
int fs_hyper_dyn_state_configure(fs_hyper_dyn_state_t state, double dt, double eta_m, const double* mass, const double* load,
                                 int64_t n_dirichlet, const int32_t* dirichlet_dofs, const double* dirichlet_values);
int fs_hyper_dyn_state_set(fs_hyper_dyn_state_t state, const double* u, const double* w, int64_t step);
int fs_hyper_dyn_state_get(fs_hyper_dyn_state_t state, double* u, double* w, int64_t* step);
int fs_hyper_dyn_start(fs_hyper_dyn_state_t state, const fs_hyper_form* form, const double* u0, const double* v0, double load_scale0,
                       double dirichlet_scale0, double dirichlet_scale1);
int fs_hyper_dyn_advance(fs_hyper_dyn_state_t state, const fs_hyper_form* form, int64_t n_steps, const double* load_scale,
                         const double* dirichlet_scale, int64_t n_receivers, const int32_t* receiver_dofs, double* traces,
                         double* energy, fs_march_info* info);
int fs_hyper_dyn_full_step(fs_hyper_dyn_state_t state, const fs_hyper_form* form, double load_scale_n, double* v_out, double* a_out);
int fs_hyper_dyn_internal_force(fs_hyper_dyn_state_t state, const fs_hyper_form* form, double* f_out, double* energy_out);

/* ---- Large-deformation elasticity (LargeDeformationSolver.py:80-135) ---------------------------------------------------------
 * Mixed CG1 (u, v, p), one Crank-Nicolson step (q; dt), F = I + grad u, J = det F, S = J (-p I + mu (B - I)) F^-T, pp = p/lambda +
 * J^2 - 1, follower loads J F^-T g on boundary facets.  The u rows are linear, du = dt (q dv - r_u) with r_u = (u - u0)/dt - q v -
 * (1-q) v0 where the displacement is free (0 where it is Dirichlet), so the Newton system is assembled for (dv, dp) only:
 *   Jr = [J_vv + dt q J_vu, J_vp; dt q J_pu, J_pp] on the CG1 block-4 space (block (v_x, v_y, v_z, p) per vertex; triangles:
 *        (v_x, v_y, -, p), the third slot an identity row), the J_xu columns of Dirichlet displacement components dropped;
 *   rhs = [-R_v + dt J_vu r_u; -R_p + dt J_pu r_u] (block layout), zero on Dirichlet v / p rows, which become identity rows.
 * u, u0: vector CG1 dof vectors (d per vertex); w, w0: block vectors (v, p) of the iterate and of the previous step.
 * dirichlet[n_vertices] (host): bits 0-2 displacement components, 3-5 velocity components, 6 pressure.
 * Facets: device cell and the cell's local vertex opposite the facet, g[n_facets][3] the load vector on the reference facet (its
 * integral is added to R_v with the sign as given).  info->residual_norm: ||(R_u, R_v, R_p)||_2 with the Dirichlet rows left out;
 * n_bad / first_bad_cell (caller's numbering, -1: none): cells with J == 0 or J not finite.  One rank; no atomics (a repeated call
 * gives the same bits). */
typedef struct fs_ld_form {
    double dt, q, mu, lambda;
    double body_force[3];       /* constant f of + int f . _v dx (the reference's sign) */
    const uint8_t* dirichlet;
    int64_t n_facets;
    const int32_t* facet_cell;
    const int32_t* facet_opposite;
    const double* facet_g;
} fs_ld_form;
typedef struct fs_ld_info {
    double residual_norm;
    int64_t n_bad;
    int64_t first_bad_cell;
} fs_ld_info;
int fs_assemble_large_deformation(fs_matrix_t Jr, fs_vector_t rhs, fs_vector_t u, fs_vector_t w, fs_vector_t u0, fs_vector_t w0,
                                  const fs_ld_form* form, fs_ld_info* info);

/* Right-hand sides of the L2 projection of the fluid stress  nu (grad u + grad u^T) - p I  onto CG1
 * (CoupledNavierStokesSolver.py:149-155, viscous_stress): b[vertex*9 + 3 i + j] = int sigma_ij phi_vertex dx for a
 * Taylor-Hood iterate w (block (u_x,u_y,u_z,p) per CG2 node).  Each of the 9 components is then one CG1 mass-matrix
 * solve (fs_assemble_matrix(mass = 1) on p1_space + fs_krylov_solve).  On triangles (2-D Taylor-Hood, third slot of the
 * block unused): b[vertex*4 + 2 i + j], four components. */
int fs_assemble_viscous_stress(fs_space_t th_space, fs_vector_t w, double nu, fs_space_t p1_space, fs_vector_t b);
/* The same with nu(p) = nu (p / p_ref)^exponent (fs_ns_form.viscosity_pressure_ref / _exponent). */
int fs_assemble_viscous_stress_nn(fs_space_t th_space, fs_vector_t w, double nu, fs_space_t p1_space, fs_vector_t b,
                                  double viscosity_pressure_ref, double viscosity_pressure_exponent);

/* SUPG part of the boundary integrals (the reference substitutes q + tau (v . grad q) in them too,
 * ScalarTransportSolver.py:296-298 with Tq): for every listed boundary facet (cell behind it, local vertex opposite)
 *   b_a += g_f * area * w_a                      (flux / Neumann / HTC ambient loads; g may be NULL)
 *   A_ab += h_f * (area / 3) * w_a, b on the facet (HTC / Robin matrices; h may be NULL)
 * for all four vertices a of the cell, w_a = tau (v . grad phi_a).  A or b may be NULL.  CG2 spaces: a runs over all dofs of
 * the cell, the load takes v . grad q_a at the facet centroid, the matrix  h tau int_F phi_b (v . grad q_a) ds  by quadrature. */
int fs_assemble_facet_supg(fs_space_t space, fs_matrix_t A, fs_vector_t b, int64_t n_facets, const int32_t* facet_cell,
                           const int32_t* facet_opposite, const double* g, const double* h, const fs_coef* velocity,
                           double supg_pe);

/* Boundary-facet integrals over an explicit facet list (the host resolves
 * ds(id) to facets).  tri[n_facets][3] local vertex ids.
 *   vector:  b_a += int g phi_a ds, g[n_facets][ncomp]  (flux / Neumann / traction,
 *            ScalarTransportSolver.py:176-200, LinearElasticitySolver.py:165-196)
 *   matrix:  A_ab += int h phi_a phi_b ds, h[n_facets]   (HTC / Robin, :201-208) */
int fs_assemble_facet_vector(fs_space_t space, int64_t n_facets, const int32_t* tri,
                             const double* g, fs_vector_t b);
int fs_assemble_facet_matrix(fs_matrix_t A, int64_t n_facets, const int32_t* tri, const double* h);

/* Replaces DirichletBC.apply(A, b) (symmetric == 0: rows -> identity, b_i = g;
 * LinearVariationalSolver, SolverBase.py:608-612) and the elimination done by
 * assemble_system (symmetric == 1: additionally b -= A[:,i] g, columns zeroed;
 * SolverBase.py:644).  dofs are local dof indices (may include ghosts); later
 * entries win on duplicates, as later BCs do in DOLFIN.  A may be NULL to set
 * only b_i = g. */
int fs_apply_dirichlet(fs_matrix_t A, fs_vector_t b, int64_t n, const int32_t* dofs,
                       const double* vals, int symmetric);

/* y = A x  (PETSc MatMult).  x has n_cols entries, y n_rows.  With a halo plan
 * attached and a communicator up, ghosts of x are refreshed first. */
int fs_spmv(fs_matrix_t A, fs_vector_t x, fs_vector_t y);

/* Matrix-free product y = K(form) x on a scalar CG1 or (round 6: constant / per-cell scalar coefficients, no advection) CG2 space over tetrahedra (what `assemble(a)` followed by MatMult
 * would give, SolverBase.py:586-590, without forming the matrix): the row-gather assembly walk with every local row
 * multiplied into x.  No Dirichlet rows (callers mask); x must carry current ghost values.  reps > 1 with
 * ms_per_launch != NULL additionally times reps launches with HIP events (mean milliseconds per product). */
int fs_operator_apply(fs_space_t V, const fs_bilinear_form* form, fs_vector_t x, fs_vector_t y, int reps,
                      double* ms_per_launch);

/* ---- Krylov (PETScKrylovSolver("cg", pc).solve, SolverBase.py:663-670) -------- */

#define FS_KSP_CG 0
#define FS_KSP_BICGSTAB 1 /* non-symmetric operators (advection); PETSc KSPBCGS, right Jacobi */
#define FS_PC_NONE 0
#define FS_PC_JACOBI 1
#define FS_PC_BLOCK_JACOBI 2 /* DG matrices only: the inverse of every cell's diagonal block, computed on the device at solve start.
                              * On a DG matrix fs_krylov_solve runs BiCGStab (right-preconditioned) and honours norm_type: with
                              * FS_NORM_PRECONDITIONED (and a preconditioner) it stops only when ||b - A x||_2 <= max(rtol ||b||_2, atol)
                              * AND ||M^-1 (b - A x)||_2 <= max(rtol ||M^-1 b||_2, atol) (bnorm / rel_residual / true_rel_residual stay
                              * in the plain norm); converged = 1 only when the TRUE residual meets the test (the recurrence restarts
                              * from b - A x while that still lowers it) */
#define FS_NORM_UNPRECONDITIONED 0 /* ||b - A x||_2 <= rtol ||b||_2 (BASELINE.json's definition) */
#define FS_NORM_PRECONDITIONED 1   /* ||D^-1 (b - A x)||_2 <= rtol ||D^-1 b||_2: PETSc's KSPCG default, robust when
                                    * constrained (identity) rows and physical rows differ by orders of magnitude */

typedef struct fs_krylov_opts {
    int method;          /* FS_KSP_CG | FS_KSP_BICGSTAB */
    int precond;         /* FS_PC_* */
    double rtol;         /* stop when ||r||_2 <= max(rtol*||b||_2, atol) */
    double atol;
    int max_iter;
    int batch;           /* iterations enqueued between host polls (0 = default 32) */
    int nonzero_guess;   /* 0: x0 = 0 (PETSc default); 1: use x on entry */
    int norm_type;       /* FS_NORM_*; the preconditioned norm needs CG + Jacobi + diagonal_scale */
    int diagonal_scale;  /* CG + Jacobi only: run on D^-1/2 A D^-1/2 (PETSc KSPSetDiagonalScale): same iterates,
                          * 25 % less vector traffic; A itself is left untouched (a scaled copy is kept) */
    int pipelined;       /* CG + Jacobi + diagonal_scale only.  1: the pipelined recurrence of Ghysels & Vanroose - the sums
                          * of an iteration are all-reduced WHILE its product runs instead of between product and update
                          * (same iterates in exact arithmetic, 112 instead of 72 B/DOF of vector traffic, attainable
                          * accuracy guarded by the same true-residual restarts); 0 / -1: the single-reduction recurrence
                          * (the default: measured on MI355X the pipelined one is the slower of the two at every size and
                          * transport tried, DESIGN.md section 5 - it is kept for communicators with a slow all-reduce) */
} fs_krylov_opts;

typedef struct fs_krylov_stats {
    int iterations;
    int converged;          /* 1 converged, 0 max_iter reached, -1 breakdown */
    double bnorm;           /* ||b||_2 (global) */
    double rel_residual;    /* recurrence ||r||/||b|| at exit */
    double true_rel_residual; /* ||b - A x||/||b|| recomputed at exit */
    double solve_ms;        /* wall time of the solve (host clock, synchronised) */
    double spmv_ms;         /* mean duration of the fused SpMV+dots kernel (HIP events) */
    double update_ms;       /* mean duration of the fused vector-update kernel */
    int64_t spmv_bytes;     /* algorithmic bytes of one SpMV: nnz*12 + n*20 */
    int row_classes;        /* > 0: the product ran in row-dictionary form with this many distinct rows (the operator of a uniform
                             * box mesh with constant coefficients: class numbers + the distinct rows in LDS instead of the value
                             * stream, verified bit for bit against the assembled values); 0: the streaming kernels */
    int fused_iteration;    /* 1: every CG iteration was ONE launch (update of iteration k + product of iteration k + 1 on a
                             * row-dictionary operator; spmv_ms is then the duration of that launch and update_ms 0); 2: a decomposed
                             * space - that launch preceded by the peer-to-peer exchange kernel (two launches per iteration;
                             * spmv_ms is the pair) */
    int classes_kept;       /* 1: the class table of the previous call on this space was kept - every row of THIS matrix was
                             * compared with its old class, bit for bit, and none differed (a steady problem solved again, a
                             * transient one with a constant step: one pass over the values instead of three); 0: the classes
                             * were found from scratch (or the streaming kernels ran) */
    int lattice_order;      /* 1: a scalar CG2 operator on a uniform box, solved in the solver's lattice order of the half grid (values,
                             * b and x permuted in and out; the API numbering is untouched): option "lattice_order" */
    int launches;           /* iterations ENQUEUED over all passes (fs_krylov_solve): those behind the one that stopped the
                             * recurrence return on the status word - launches - iterations of them, a few microseconds each */
    int product_kind;       /* kernel family of the solve's products (fs_last_product_kind): 0 streaming, 1 row-dictionary work items
                             * (also inside the one-launch iteration), 2 lattice tiles, 3 marching windows of a P1 box, 4 block rows,
                             * 5 marching windows of a CG2 box in lattice order, 6 DG cell blocks (k_dg_spmv) */
} fs_krylov_stats;

int fs_krylov_solve(fs_matrix_t A, fs_vector_t b, fs_vector_t x, const fs_krylov_opts* opts,
                    fs_krylov_stats* stats);
/* ||r_k||_2^2 history of the last solve, k = 0..iterations. */
int fs_krylov_history(double* out, int capacity, int* count);

/* Time |reps| back-to-back launches of the SpMV kernel with HIP events on the
 * library's stream; returns mean milliseconds per launch.  reps > 0: bare y = A x;
 * reps < 0: the CG flavour fused with the three dot products (y plays r). */
int fs_spmv_benchmark(fs_matrix_t A, fs_vector_t x, fs_vector_t y, int reps, double* ms_per_launch);

/* y = A x (MatMult, behind KSPSolve at SolverBase.py:663-670) through the ROW-DICTIONARY form of the product where the rows of A
 * repeat (a uniform box mesh with constant coefficients): the classes are found from A's current values inside this call (or
 * kept from the previous call on the same space, where every row of A still equals its old class),
 * every row is verified against its class, and no later call multiplies from the table without verifying its own matrix against it.  *row_classes = number of distinct
 * rows used, 0 = the rows do not repeat and the streaming product ran.  Both forms give the same bits as fs_spmv. */
int fs_spmv_dictionary(fs_matrix_t A, fs_vector_t x, fs_vector_t y, int* row_classes);

/* Which kernel the LAST product launched by this process went through (MatMult, SolverBase.py:663-670; a diagnostic - PETSc's
 * analogue is the -log_view line of MatMult): 0 streaming SELL / DIA kernels, 1 row-dictionary work items (k_dict_spmv), 2 lattice
 * tiles of a CG2 box (k_lattice_spmv), 3 marching windows of a P1 box (k_box_spmv, round 6: options "box_spmv" 1 / 0 and
 * "box_min_rows", default 1 500 000), 4 block rows (k_dict_spmv3; k_sell_spmv4_* on 4 x 4-block operators), 5 marching windows of a CG2 box in lattice order
 * (k_lat_march, round 6: option "lattice_march" 1 / 0), 6 DG cell blocks (k_dg_spmv).  The one-launch iteration k_dict_cg_iter does not count as a product here. */
int fs_last_product_kind(void);
/* Form of the one-launch CG iteration (k_dict_cg_iter) in the LAST solve of this process, 0 if it did not run: bit 0 = p and x updated every
 * second launch (option "cg_pair"), bit 1 = the dot weights came from the table by row class (every row of the solve's weight vector
 * equalled its class's entry bit for bit) and not from the weight vector. */
int fs_last_iteration_form(void);
/* ... and what option "cg_guard" did in that solve, 0 if nothing: bit 0 = guarded work vectors, no edge-item path, bit 1 = with them, the own
 * rows taken from the centre run of the space's one plan (Kuhn box) and the z run neither loaded nor multiplied.  (A word of its own:
 * callers of fs_last_iteration_form compare that word with the two bits it has.) */
int fs_last_iteration_guard(void);
/* ... and how many of the seven runs of a Kuhn-box row its LIGHT / PAIR launches left out because every class row of the solve's dictionary
 * held nothing above 2^-53 of its unit diagonal there (option "cg_zero_runs"): 0 or 2.  A word of its own: the two above keep their values. */
int fs_last_iteration_runs(void);

/* ---- smoothed-aggregation AMG (PETScPreconditioner("petsc_amg") + set_near_nullspace,
 *      SolverBase.py:643-672; Chebyshev/Jacobi level smoother as the PETScOptions there ask) ---- */

typedef struct fs_amg_s* fs_amg_t;

typedef struct fs_amg_opts {
    double strength_threshold; /* theta of |A_ij|^2 > theta^2 |A_ii||A_jj| (block Frobenius norms); 0 = 0.05,
                                * negative = every coupling above rounding noise (1e-8) */
    int max_levels;            /* 0 = 10 */
    int coarse_size;           /* stop coarsening at this many dofs; 0 = 500 */
    int smoother_steps;        /* Chebyshev steps per pre/post smoothing; 0 = 2 (PETSc mg_levels_ksp_max_it) */
    int eig_steps;             /* power-iteration steps before the Rayleigh quotient of the eigenvalue estimate; 0 = 15 */
    int rigid_body_modes;      /* nullspace == NULL and a 3-vector CG1 space: build the six rigid-body modes of
                                * build_nullspace() (SolverBase.py:674-706) on the device from the node coordinates */
} fs_amg_opts;

/* Build the hierarchy for the assembled (Dirichlet-eliminated, SPD) matrix.  nullspace: host array
 * [n_nullspace][n_dofs] of near-null-space vectors (the rigid-body modes of build_nullspace(),
 * SolverBase.py:674-706), or NULL = one constant per component.  The matrix must outlive the
 * hierarchy and keep its values.  On a space with ghost nodes the hierarchy is built on this rank's diagonal
 * block (ghost columns dropped): fs_amg_solve is then CG on the distributed operator with the rank-local
 * V-cycles as non-overlapping additive Schwarz preconditioner. */
int fs_amg_setup(fs_matrix_t A, int n_nullspace, const double* nullspace, const fs_amg_opts* opts, fs_amg_t* out);
/* Distributed fine level under a replicated hierarchy (several GPUs; PETSc's GAMG under mpirun keeps the fine level distributed
 * and agglomerates the coarse ones, SolverBase.py:643-672 + :634).  M was set up on the UNDECOMPOSED operator, identically on
 * every rank; A_local holds this rank's rows of the decomposed operator (halo plan on its space); owned_global_nodes[i] = the
 * node, in the undecomposed space, of local owned node i.  Afterwards fs_amg_apply / fs_amg_solve smooth, restrict and prolong
 * level 0 on this rank's rows (ghost refresh before every fine product, the restricted right-hand side summed over the ranks)
 * and apply levels >= 1 as they are: the preconditioner - and the iteration count - of one GPU, with the fine-level work
 * divided by the number of ranks.  COLLECTIVE in its use (every rank attaches its part before the first solve).  A second call
 * on a hierarchy that has its fine level attached swaps in A_local - a matrix on the SAME decomposed space holding the same
 * operator (a hierarchy kept over several solves multiplies with the caller's current matrix, not the first one). */
int fs_amg_attach_distributed_fine(fs_amg_t M, fs_matrix_t A_local, int64_t n_owned_nodes, const int32_t* owned_global_nodes);
int fs_amg_destroy(fs_amg_t amg);
int fs_amg_info(fs_amg_t amg, int* n_levels, double* operator_complexity, double* grid_complexity, double* setup_ms);
int fs_amg_level_info(fs_amg_t amg, int level, int64_t* n_nodes, int* block_size, int64_t* nnz_blocks,
                      int64_t* p_nnz_blocks, int* p_block_cols, double* lambda_max);
/* which: 0 = level operator A (block CSR, blocks row-major), 1 = prolongator to this level from the
 * next, 2 = near-null space [n_dofs][nb] (val only), 3 = the dense inverse of the coarsest operator
 * that the V-cycle applies there ([n_dofs][n_dofs] row-major, val only, level = the last one;
 * FS_ERR_UNSUPPORTED when the hierarchy has none: a single level, or more than 2500 rows on the
 * coarsest, where the cycle runs Chebyshev sweeps instead; val == NULL only asks whether there is
 * one), 4 = the aggregate of every node of a level with a prolongator (col only: n_nodes int32, the
 * block column of the tentative prolongator, -1 = in no aggregate because the node has no strong
 * coupling; an error on a level without a prolongator).  Test/inspection hook. */
int fs_amg_level_get(fs_amg_t amg, int level, int which, int32_t* rowptr, int32_t* col, double* val);
/* z = M r: one V-cycle from a zero guess (PCApply). */
int fs_amg_apply(fs_amg_t amg, fs_vector_t r, fs_vector_t z);
/* CG preconditioned by the V-cycle (PETScKrylovSolver("cg", pc).solve, SolverBase.py:660-670);
 * uses rtol, atol, max_iter, nonzero_guess and norm_type of the options. */
int fs_amg_solve(fs_amg_t amg, fs_vector_t b, fs_vector_t x, const fs_krylov_opts* opts, fs_krylov_stats* stats);

/* ---- block eigensolver (SLEPcEigenSolver, LinearElasticitySolver.py:283-310) ---------------------------------------------
 * Lowest modes of K phi = lambda M phi by LOBPCG; the reference asks SLEPc for its default (largest magnitude, K alone), this one for
 * the n_modes smallest eigenvalues of the pencil on the free dofs ("differs from the reference").  One rank. */

/* Y[j] = A X[j] for j < m (the MatMult of every column of the eigensolver's block, LinearElasticitySolver.py:283-310) in one pass over
 * A's values per chunk of columns; block sizes 2 and 3.  Unmasked; each Y[j] equals fs_spmv(A, X[j], Y[j]) bit for bit. */
int fs_spmv_multi(fs_matrix_t A, int m, const fs_vector_t* X, fs_vector_t* Y);

/* G[i * q + j] = X[i] . Y[j] (the block inner products of SLEPc's BV, behind LinearElasticitySolver.py:283-310); all vectors of
 * one length.  Deterministic: the same inputs give the same bits. */
int fs_vector_gram(int p, const fs_vector_t* X, int q, const fs_vector_t* Y, double* G);

typedef struct fs_eigen_opts {
    int n_modes;         /* wanted eigenpairs, 1 .. 32 (SLEPcEigenSolver.solve(n), LinearElasticitySolver.py:298) */
    int block;           /* block size m; 0 = min(2 n_modes, n_modes + 8); at most 40 */
    double tol;          /* stop when every wanted column has ||K x - lambda M x||_2 <= tol lambda_shifted ||M x||_2 */
    int max_iter;
    double shift;        /* sigma >= 0: K holds K + sigma M; the eigenvalues returned are lambda - sigma */
    uint64_t seed;       /* of the pseudo-random start block */
} fs_eigen_opts;

typedef struct fs_eigen_stats {
    int iterations;
    int n_converged;            /* wanted columns that met the test, on products recomputed from X */
    double max_rel_residual;    /* largest relative residual of the wanted columns */
    double solve_ms;            /* wall time (host clock, synchronised) */
    double block_product_ms;    /* HIP events: block products with K and M */
    double gram_ms;             /* ... Gram matrices (with their download) */
    double precond_ms;          /* ... V-cycles or Jacobi */
} fs_eigen_stats;

/* SLEPcEigenSolver(K).solve (LinearElasticitySolver.py:283-310) for the pencil (K, M): K and M on one space, K Dirichlet-eliminated
 * or not (constrained rows and columns are masked out), precond = an fs_amg_setup hierarchy of K or NULL (Jacobi).  constrained:
 * the n_constrained dofs every mode is zero at.  eigenvalues[n_modes] ascending; modes[n_modes] (caller's vectors of >= n_dofs_owned
 * entries) M-orthonormal. */
int fs_eigen_solve(fs_matrix_t K, fs_matrix_t M, fs_amg_t precond, int64_t n_constrained, const int32_t* constrained,
                   const fs_eigen_opts* opts, double* eigenvalues, fs_vector_t* modes, fs_eigen_stats* stats);

/* ---- linear (eigenvalue) buckling --------------------------------------------------------------------------------------------
 * No counterpart in the reference ("differs from the reference"): the factors lambda > 0 of the reference load at
 * which (K + lambda K_G) phi = 0, K_G the geometric stiffness of the static solution's stress.  Vector CG1 spaces on tetrahedra
 * (3 components) or on triangles in plane strain (2 components); one rank. */

/* K_G[(a,i),(b,j)] = delta_ij sum_cells |c| grad N_a . sigma_c grad N_b with sigma_c = lambda tr(eps) I + 2 mu eps of the displacement
 * u (>= n_dofs_local entries), constant per P1 cell.  Lame coefficients: (mu, lambda), or lame_cells != NULL: [n_cells][2] pairs
 * (mu, lambda) per cell in device cell order, as FS_COEF_CELL_LAME of fs_assemble_matrix (mu and lambda are ignored then).  KG: a
 * matrix of the space; every node-pair block becomes s I (off-diagonal block entries exactly 0.0).  No atomics: two calls give the
 * same bits.  cell_stress_out (may be NULL): the stress per cell in device cell order, 6 doubles (xx, yy, zz, xy, xz, yz) on
 * tetrahedra, 4 (xx, yy, zz, xy) in plane strain - sigma_zz = lambda tr(eps) there, which does not enter K_G. */
int fs_assemble_geometric_stiffness(fs_space_t space, double mu, double lambda, const double* lame_cells, fs_vector_t u, fs_matrix_t KG,
                                    double* cell_stress_out);

/* YK[j] = K X[j] and YG[j] = KG X[j] for j < m in one pass over the pattern per chunk of columns: the column indices and X are
 * gathered once, and KG - whose blocks must be s I, as fs_assemble_geometric_stiffness leaves them; FS_ERR_INVALID otherwise - is read
 * from a copy of one double per node pair.  Unmasked.  YK[j] equals fs_spmv_multi(K) bit for bit; YG[j] equals fs_spmv_multi(KG)
 * as numbers for finite X (the block product adds exact zeros, which can only change the sign of a zero). */
int fs_spmv_multi_pencil(fs_matrix_t K, fs_matrix_t KG, int m, const fs_vector_t* X, fs_vector_t* YK, fs_vector_t* YG);

/* Mean milliseconds (HIP events, after 3 warm-up launches, over reps launches) of one fused pencil product of m columns of a seeded
 * block, and of the two fs_spmv_multi block products (K, then KG) it replaces, the kernels only. */
int fs_spmv_multi_pencil_benchmark(fs_matrix_t K, fs_matrix_t KG, int m, int reps, double* fused_ms, double* two_pass_ms);

typedef struct fs_buckling_opts {
    int n_modes;         /* wanted buckling factors, 1 .. 32 */
    int block;           /* block size m; 0 = min(2 n_modes, n_modes + 8); at most 40 */
    double tol;          /* stop when every wanted column has ||K_G x - nu K x||_2 <= tol |nu| ||K x||_2 */
    int max_iter;
    uint64_t seed;       /* of the pseudo-random start block */
    int two_pass;        /* 0: K S and K_G S by the fused pencil product; 1: by two block products (the kernels of fs_spmv_multi) */
} fs_buckling_opts;

typedef struct fs_buckling_stats {
    int iterations;
    int n_converged;            /* wanted columns that met the test, on products recomputed from X */
    double max_rel_residual;    /* largest relative residual of the wanted columns */
    int n_negative;             /* Ritz values nu < 0 among the block's m at the end: the buckling modes the block holds */
    double solve_ms;            /* wall time (host clock, synchronised) */
    double block_product_ms;    /* HIP events: products with K and K_G */
    double gram_ms;             /* ... Gram matrices (with their download) */
    double precond_ms;          /* ... V-cycles or Jacobi */
} fs_buckling_stats;

/* The n_modes smallest positive lambda of (K + lambda K_G) phi = 0 on the dofs outside `constrained`, by the LOBPCG of fs_eigen_solve on
 * K_G phi = nu K phi (lambda = -1 / nu for the most negative nu).  K: Dirichlet-eliminated or not (constrained rows and columns are
 * masked out); KG: as assembled, NOT Dirichlet-eliminated (its blocks must be s I); precond: an fs_amg_setup hierarchy of K, or NULL
 * (the Jacobi diagonal of K).  factors[n_modes] ascending; modes[n_modes] (caller's vectors of >= n_dofs_owned entries) K-orthonormal.
 * When the iteration converges with fewer than n_modes negative nu: FS_ERR_NUMERIC, "the reference load produces only N buckling
 * mode(s)" (N = 0: nothing buckles under this load), with stats filled. */
int fs_buckling_solve(fs_matrix_t K, fs_matrix_t KG, fs_amg_t precond, int64_t n_constrained, const int32_t* constrained,
                      const fs_buckling_opts* opts, double* factors, fs_vector_t* modes, fs_buckling_stats* stats);

/* ---- anisotropic linear elasticity ----------------------------------------------------------------------------------------------
 * No counterpart in the reference, whose to-do list names it ("anisotropy needs rank 4 tensor"; INTEGRATION.md, "differs from the
 * reference").  Vector CG1 spaces on tetrahedra (3 components) or on triangles in plane strain (2 components); one rank; no DG.
 * fs_bilinear_form is unchanged: the material has a struct of its own. */
typedef struct fs_aniso_material {
    int64_t n_materials;            /* >= 1 */
    const double* stiffness;        /* [n_materials][21]: upper triangle, row-major, of the symmetric 6x6 D in the library's tensor
                                     * order (xx, yy, zz, xy, xz, yz) acting on (e_xx, e_yy, e_zz, 2e_xy, 2e_xz, 2e_yz): D_IJ = C_ikjl */
    const int32_t* material_of_cell;/* [n_cells], device cell order; NULL: every cell is material 0 - or, when n_materials == n_cells,
                                     * the identity map: cell c has material c (a fully per-cell C).  Any other n_materials with a
                                     * NULL index is refused. */
    const double* frame;            /* [n_cells][9] row-major rotation R (columns = material axes in global coordinates),
                                     * C_global = (R x R x R x R) C_material; NULL: identity everywhere */
} fs_aniso_material;
/* All arrays are host arrays.  Checked before anything is enqueued (FS_ERR_INVALID): finite entries, the range of material_of_cell,
 * n_materials against the mesh when the index is NULL; in plane strain also that every D is monoclinic about z (D[I][xz] = D[I][yz]
 * = 0 for I in xx, yy, zz, xy) and every frame a rotation about z.  Symmetry is in the storage; positive definiteness and the
 * orthogonality of the frames are the caller's to check (LinearElasticitySolver does).  The kernels never rotate C: they rotate the
 * gradients into the material axes and the block back, K_ab = R (V ghat_a . C . ghat_b) R^T with ghat = R^T g. */

/* A (+)= int eps(v) : C : eps(u) dx + mass u.v; mass: NULL, FS_COEF_NONE, FS_COEF_CONST or FS_COEF_CELL, with the mass arithmetic of
 * fs_assemble_matrix.  One thread per stored block over its sources in ascending order, no atomics: two calls give the same bits, and
 * on a box mesh translated stencils give equal rows (the snapped geometry of the isotropic kernel).  Enqueues and does not wait, as
 * fs_assemble_matrix. */
int fs_assemble_anisotropic(fs_matrix_t A, const fs_aniso_material* mat, const fs_coef* mass, int add);

/* sigma = C : (eps(u) - eps*) per cell in device cell order: 6 doubles (xx, yy, zz, xy, xz, yz) on tetrahedra, 4 (xx, yy, zz, xy) in
 * plane strain.  eigenstrain: [n_cells][6 or 4] tensor components (not engineering shears) in global axes, or NULL; u (>= n_dofs_local
 * entries) may be NULL: the stress of -eps* alone.  cell_stress_out (may be NULL): the stress, downloaded.  vm_rhs with p1_space (both
 * or neither): the right-hand side int sqrt(3/2 s:s) phi_a dx of the von Mises L2 projection onto the scalar CG1 space of the mesh,
 * gathered per vertex in ascending cell order as fs_assemble_von_mises does (2-D: its deviator convention, s = sigma_2x2 - tr / 3 I). */
int fs_anisotropic_stress(fs_space_t space, fs_vector_t u, const fs_aniso_material* mat, const double* eigenstrain,
                          double* cell_stress_out, fs_space_t p1_space, fs_vector_t vm_rhs);

/* b (+)= int (C : eps*) : grad v dx (>= n_dofs_owned entries): the per-cell stress kernel of fs_anisotropic_stress into a device
 * array, then the stored-stress force gather the inelastic solvers use. */
int fs_assemble_anisotropic_load(fs_space_t space, const fs_aniso_material* mat, const double* eigenstrain, fs_vector_t b, int add);

/* ---- frictionless contact and sliding supports --------------------------------------------------------------------------------
 * No counterpart in the reference, which lists the boundary condition as not implemented ("differs from the
 * reference").  Vector CG1 spaces on tetrahedra (3 components) or on triangles in plane strain (2 components); one rank.
 *
 * Every framed node a has a unit normal n_a and the Householder reflector H_a = I - 2 v v^T / v^T v, v = n_a + s e_k, k the last
 * axis, s = sgn(n_k) (sgn(0) = +1): symmetric, its own inverse, H_a e_k = sigma_a n_a with sigma_a = -s.  With H = blockdiag(H_a)
 * (the identity on every other node) and u' = H u, the normal displacement of node a is the one dof u'[d a + k] = sigma_a n_a . u_a:
 * the constraint n_a . u_a = value_a is a component Dirichlet condition on K' = H K H, b' = H b (fs_apply_dirichlet). */
typedef struct fs_contact_s* fs_contact_t;

/* The frames and the active-set state of n nodes (strictly ascending node ids of the space): normals [n][d] (any length > 0,
 * normalised here; FS_ERR_INVALID on a zero or non-finite one), values [n] (the clearance g_a along n_a of a contact node, the
 * prescribed normal displacement of a bilateral one), bilateral [n] (non-zero: a sliding support, always active), active [n] (the
 * first active set of the contact nodes).  Held on the device: nodes, reflectors, sigma, values, the bilateral flags, the active
 * flags, and lambda and the penetration of the last fs_contact_update. */
int fs_contact_create(fs_space_t space, int64_t n, const int32_t* nodes, const double* normals, const double* values,
                      const int32_t* bilateral, const int32_t* active, fs_contact_t* out);
int fs_contact_destroy(fs_contact_t state);
/* active [n], lambda [n], penetration [n] (each may be NULL) as the last fs_contact_update left them */
int fs_contact_get(fs_contact_t state, int32_t* active, double* lambda, double* penetration);

/* A <- H A H in place on the block values (block size 2 or 3): the owner of block (a, b) writes H_a A_ab H_b.  The pattern is
 * unchanged, no atomics, and a block with neither node framed is not written. */
int fs_matrix_rotate_nodes(fs_matrix_t A, fs_contact_t frames);
/* x <- H x (>= n_dofs_owned entries): right-hand sides, initial guesses, near-null-space vectors, and the way back u = H u'. */
int fs_vector_rotate_nodes(fs_vector_t x, fs_contact_t frames);

/* One primal-dual active-set update from the solution u' (>= n_dofs_local entries) of the system constrained on the current active
 * set, with the UNCONSTRAINED K' and b': for every node of the state rho = (K' u' - b')[d a + k] (the row of the normal dof only,
 * summed in storage order: the same bits on every call), lambda_a = -sigma_a rho, the penetration p_a = sigma_a u'[d a + k] - value_a,
 * and the next flag  active ? lambda_a > 0 : p_a > 0  (an exact zero releases, or stays out); bilateral nodes stay active.
 * counts[0]: flags that changed, counts[1]: flags now active - through two words of pinned host memory, one read per call. */
int fs_contact_update(fs_contact_t state, fs_matrix_t Kprime, fs_vector_t uprime, fs_vector_t bprime, int32_t* counts);

/* ---- Taylor-Hood Navier-Stokes (CoupledNavierStokesSolver.py:288-381, 215-245, 492-528) -------------
 * Unknowns: one block (u_x, u_y, u_z, p) per CG2 node of fs_space_create(mesh, FS_FAMILY_CG, 2, 4); the
 * pressure is CG1, the pressure slot of an edge node is a dummy unknown with a unit row. */

typedef struct fs_ns_form {
    double kinematic_viscosity; /* nu: 2 nu eps(u):eps(v) */
    double density;             /* rho: -(p/rho) div v + (q/rho) div u */
    double inv_dt;              /* 1/dt of the backward-Euler term (F_transient), 0 = steady */
    double body_force[3];       /* f of -f.v (acceleration, "just gravity, without * rho") */
    int convection;             /* (grad(u) u0).v with u0 = velocity part of w0 */
    int newton;                 /* add (grad(u0) u).v to J and (grad(u0) u0).v to g: derivative(action(F, w0)) */
    double mesh_velocity[3];    /* ALE frame (reference_frame_settings, CoupledNavierStokesSolver.py:321-329): the advecting
                                 * velocity is u0 - mesh_velocity, i.e. the term is (grad(u) (u0 - w)).v; constant vector.
                                 * Written for the new iterate, the Newton right-hand side keeps (grad(u0) u0).v. */
    int g2_mode;                /* G2 streamline term of advection_settings (CoupledNavierStokesSolver.py:334-363):
                                 * F -= delta1 (a.grad u).(a.grad v) dx, a the advecting velocity, h = 2 circumradius;
                                 * 0 off, 1: delta1 = kappa1 h^2 (Re <= 1), 2: kappa1/2 h/|a| (steady) or
                                 * kappa1/2 / sqrt(1/dt^2 + 1/(|a|^2 h^2)) (inv_dt > 0).  Enters J with a frozen at w0 (the
                                 * system is written for the new iterate, so g is unchanged and J w - g is the exact residual). */
    double g2_kappa1;
    double viscosity_pressure_ref;      /* > 0: the non-Newtonian law of CoupledNavierStokesSolver.viscosity (:194-213, the branch */
    double viscosity_pressure_exponent; /* without a temperature): nu(p) = nu (p / p_ref)^exponent with the pressure of w0 (needs
                                         * w0; Picard in the viscosity - J w - g stays the exact residual).  0: Newtonian. */
} fs_ns_form;

/* The non-Newtonian laws of CoupledNavierStokesSolver.viscosity (CoupledNavierStokesSolver.py:194-213), attached to the
 * Taylor-Hood space and used by every routine that evaluates nu on it (fs_assemble_navier_stokes, the pressure-boundary traction
 * term, fs_assemble_viscous_stress*), in place of the (p_ref, exponent) pair those calls carry:
 *   kind 1  nu (p / pressure_ref)^pressure_exponent                                          (:205-207, no temperature)
 *   kind 2  nu (1 + pressure_coef p / pressure_ref) (1 - temperature_coef T / temperature_ref)   (:199-203, solving_temperature)
 * p: the pressure of the state w0 the call linearises at; temperature: CG1 field stored like the pressure inside w0 - one value per
 * LOCAL NODE of the Taylor-Hood space, read at the vertex nodes only (one GPU: the vertices are the first nodes; a decomposed space
 * orders owned vertices, owned edges, ghost vertices, ghost edges).  The vector is read at assembly time - keep it alive and current;
 * nothing is copied.  law = NULL or kind 0 detaches. */
typedef struct fs_viscosity_law {
    int kind;
    double pressure_ref, pressure_exponent;
    double pressure_coef, temperature_coef, temperature_ref;
    fs_vector_t temperature;
} fs_viscosity_law;
int fs_space_set_viscosity_law(fs_space_t th_space, const fs_viscosity_law* law);

/* J <- linearised operator at w0, g <- right-hand side such that J w_new = g is the Newton (or Picard) step
 * written for the new iterate.  w_prev: previous time step (may be NULL when inv_dt = 0). */
int fs_assemble_navier_stokes(fs_matrix_t J, fs_vector_t g, fs_vector_t w0, fs_vector_t w_prev, const fs_ns_form* form);

/* Pressure boundaries, added to J and g after fs_assemble_navier_stokes and before the Dirichlet rows:
 *   F += inner(p_b n, v) ds - nu inner((grad(u) + grad(u)^T) n, v) ds   (CoupledNavierStokesSolver.py:449-453)
 * facet_cell / facet_opposite: the cell behind each boundary facet and the local vertex opposite to it;
 * facet_value: p_b per facet, NULL = the pressure 'farfield' type (traction term only, :459-460). */
int fs_assemble_ns_pressure_boundary(fs_matrix_t J, fs_vector_t g, int64_t n_facets, const int32_t* facet_cell,
                                     const int32_t* facet_opposite, const double* facet_value, double kinematic_viscosity);
/* The same with the pressure-dependent viscosity of fs_ns_form (w0: the state whose pressure enters nu; ref 0 = off) and,
 * with values_per_facet = 3, a boundary pressure that varies over the facet: facet_value[f][k] = p_b at the facet's k-th
 * vertex in the order of the cell's local vertices (the opposite one left out) - the P1 interpolant DOLFIN evaluates a
 * degree-1 Expression with; values_per_facet = 1: one value per facet. */
int fs_assemble_ns_pressure_boundary_nn(fs_matrix_t J, fs_vector_t g, int64_t n_facets, const int32_t* facet_cell,
                                        const int32_t* facet_opposite, const double* facet_value, double kinematic_viscosity,
                                        fs_vector_t w0, double viscosity_pressure_ref, double viscosity_pressure_exponent,
                                        int values_per_facet);

typedef struct fs_saddle_opts {
    double rtol, atol;          /* on ||g - J w||_2 (relative to ||g||_2) */
    int max_iter;               /* 0 = 600 */
    int restart;                /* FGMRES restart length, 0 = 60 */
    double kinematic_viscosity, density, inv_dt; /* of the Schur-complement approximation */
    int velocity_sweeps;        /* Jacobi sweeps standing in for A^-1, 0 = 1 */
    double inner_rtol;          /* of the pressure Laplacian / mass CG solves, 0 = 1e-2 */
    int nonzero_guess;
    /* Appended; zero / NULL keeps the Taylor-Hood preconditioner above.  block_upper = 1: J is the reduced large-deformation
     * operator of fs_assemble_large_deformation (CG1 block-4 space) and the preconditioner is the right, block upper triangular
     * [A J_vp; 0 S]^-1 with S = schur_scale Mp (Mp: CG1 pressure mass matrix, 5 Chebyshev steps) and A^-1 one V-cycle of a0_amg
     * (3-D) or, without a hierarchy, Jacobi-CG on a0 to a0_rtol (0 = 1e-2).  a0: vector CG1 operator (d components on the same
     * mesh) standing in for the velocity block.  Kp, Kp_amg and the Taylor-Hood fields are not used then. */
    int block_upper;
    fs_matrix_t a0;
    fs_amg_t a0_amg;
    double a0_rtol;
    double schur_scale;
} fs_saddle_opts;

/* Restarted FGMRES on the coupled system (the reference lets PETSc LU do this, SolverBase.py:615-626),
 * right-preconditioned by [A 0; D S]^-1 with the Cahouet-Chabard Schur complement
 * S^-1 = rho^2 ((1/dt) Kp^-1 + nu Mp^-1).  Kp: CG1 stiffness matrix (coefficient 1) with the pressure
 * Dirichlet dofs eliminated, may be NULL when inv_dt = 0; Kp_amg: optional hierarchy of Kp (fs_amg_setup) - one
 * V-cycle then stands in for Kp^-1 instead of an inner CG solve; Mp: CG1 mass matrix.
 * Several GPUs (J, Kp, Mp on decomposed spaces): the multi-dot sums are all-reduced, the halo of the preconditioned
 * vector is exchanged twice per iteration, M_p^-1 acts on the rank-local block; Kp_amg is either the hierarchy of the
 * GLOBAL pressure Laplacian held by every rank (its row count differs from the owned vertices: the pressure
 * residual is all-reduced into the global vector and the V-cycle replicated - same operator as on one GPU) or a
 * rank-local hierarchy (then an inner additive-Schwarz CG solve to inner_rtol). */
int fs_saddle_solve(fs_matrix_t J, fs_matrix_t Kp, fs_amg_t Kp_amg, fs_matrix_t Mp, fs_vector_t b, fs_vector_t x,
                    const fs_saddle_opts* opts, fs_krylov_stats* stats);

typedef struct fs_saddle_cycle_info {
    int restart;            /* m: the restart length the workspace was built for */
    int columns_used;       /* kuse: iterations of the cycle that entered the update of x */
    int second_passes;      /* iterations of the cycle whose second Gram-Schmidt pass ran (an iteration enqueued ahead counts) */
    int64_t n_owned;        /* owned rows of the operator: the length of every V_k and Z_k returned */
    double vel_lmax;        /* lambda_max(D^-1 A) of the velocity block as the last velocity_sweeps > 1 solve estimated it */
} fs_saddle_cycle_info;

/* The state of the LAST FGMRES cycle of the most recent fs_saddle_solve call, copied to host arrays; every array may be
 * NULL.  V[(columns_used + 1)][n_owned]: the Arnoldi basis; Z[columns_used][n_owned]: the preconditioned vectors, owned rows;
 * H[(restart + 1)][restart] row-major: the Hessenberg matrix after the Givens rotations (upper triangular R in its first
 * columns_used columns); cs, sn[restart]: the rotations; gamma[restart + 1]: the rotated right-hand side, |gamma[columns_used]|
 * the recurrence residual the cycle stopped on; y[restart]: the NEGATIVE of the least-squares solution, as the update
 * kernel subtracts.  Column columns_used of H and entry columns_used of cs and sn may hold the iteration that was enqueued
 * ahead of the stopping test and never used: that iteration has then also rotated gamma[columns_used] on into
 * gamma[columns_used + 1], and the recurrence residual is the norm of the two (a cycle that ended at max_iter or at the
 * restart length has no such iteration).  Entries beyond are left over from earlier cycles.  Makes no launch, only
 * device-to-host copies, and leaves the solver's state alone.  FS_ERR_UNSUPPORTED when that call ran no cycle (or none was made).
 * Test/inspection hook. */
int fs_saddle_last_cycle(fs_saddle_cycle_info* info, double* V, double* Z, double* H, double* cs, double* sn, double* gamma,
                         double* y);

/* ---- multi-GPU (MPI inside PETSc/DOLFIN under mpirun; SolverBase.py:102-118, 634) */

#define FS_UNIQUE_ID_BYTES 128
int fs_comm_get_unique_id(char id[FS_UNIQUE_ID_BYTES]); /* rank 0, then broadcast out of band */
int fs_comm_init(int n_ranks, int rank, const char id[FS_UNIQUE_ID_BYTES]);
int fs_comm_info(int* n_ranks, int* rank);
int fs_comm_allreduce_sum(double* host_inout, int n); /* utility: host scalars */
/* All-gather of host arrays: every rank contributes n_send <= n_max doubles; recv [n_ranks][n_max] (padding undefined).
 * One ncclAllGather; the solver API gathers the owned parts of a solution with it. */
int fs_comm_allgather(const double* host_send, int64_t n_send, int64_t n_max, double* host_recv);
int fs_comm_finalize(void);

/* Halo plan of a space (PETSc VecScatter ghost update): for each neighbour the
 * owned local dofs to send (concatenated in send_idx) and the number of ghosts
 * received; ghosts are stored after the owned dofs, neighbour by neighbour in
 * the order given. */
int fs_space_set_halo(fs_space_t space, int n_neighbors, const int32_t* neighbor_ranks,
                      const int64_t* send_counts, const int32_t* send_idx,
                      const int64_t* recv_counts);
/* Refresh the ghost entries of a local vector (n_dofs_local long). */
/* The same with an explicit scatter list: the k-th value received from a neighbour goes to local dof recv_idx[k]
 * (>= the owned dofs).  For layouts whose ghosts are not grouped by owner, e.g. CG2 nodes
 * [owned vertices | owned edges | ghost vertices | ghost edges]. */
int fs_space_set_halo_indexed(fs_space_t space, int n_neighbors, const int32_t* neighbor_ranks, const int64_t* send_counts,
                              const int32_t* send_idx, const int64_t* recv_counts, const int32_t* recv_idx);
int fs_halo_exchange(fs_space_t space, fs_vector_t v);
/* Opt-in ghost refresh WITHOUT the library in the data path, for the ranks of one node: every rank owns a fine-grained
 * receive buffer and arrival flags, its neighbours map them through hipIpc, a kernel gathers the values a neighbour
 * needs and stores them straight into that neighbour's buffer (over xGMI), then releases a sequence number; the
 * receiver's kernel waits for the sequence numbers of all its neighbours and fills the ghost entries.  Same place in
 * the iteration as the grouped ncclSend / ncclRecv it replaces (PETSc's VecScatter behind MatMult,
 * SolverBase.py:634 under mpirun), about a third of its latency on MI355X.
 * The call ends with a self-test of the mapped buffers (an all-reduce and a ghost refresh of known values, 0.5 s time-out)
 * whose outcome the ranks agree on: FS_ERR_COMM on every rank if any of them saw a wrong or missing value.
 * COLLECTIVE over the communicator: every rank calls it for its space in the same order; enable = 0 turns it off
 * (required before fs_space_set_halo replaces the plan).  FS_ERR_COMM without a communicator.
 * Destroying a space with the exchange still on frees buffers its neighbours have mapped: do it on every rank at the same
 * point of the program (after a solve returned no rank has a store in flight), or turn the exchange off first. */
int fs_space_enable_p2p_halo(fs_space_t space, int enable);
/* Mean latency (ms) of the two collectives of a distributed CG iteration as the solver issues them - the 3-double
 * ncclAllReduce behind VecDot (SolverBase.py:634 under mpirun) and the ghost refresh of this space's halo plan behind
 * MatMult's VecScatter - over `reps` back-to-back calls (HIP events).  Collective; zeros on one rank. */
int fs_comm_benchmark(fs_space_t space, int reps, double* allreduce_ms, double* halo_ms);

#ifdef __cplusplus
}
#endif
#endif /* FENICSSOLVER_AMD_H */
