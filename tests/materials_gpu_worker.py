"""Worker of tests/test_gpu_elasticity_materials.py: one rank of a multi-rank run whose ranks SHARE ONE GPU (launched with
--devices 0,0,..; FS_RCCL_PATH = tests/shim/libfakerccl.so).  Started by fenicssolver_amd.launch.
Writes what rank 0 holds to the .npz named on the command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fenicssolver_amd import parallel    # noqa: E402

out_path, case = sys.argv[1], sys.argv[2]
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
result = {}

if case == "cantilever":
    # the two-region P1 cantilever on the replicated mesh: solve_amg, then the von Mises projection
    import test_gpu_elasticity_materials as T
    solver = T._cantilever(n=(36, 6, 6))
    u = solver.solve()
    assert solver.function_space.localizer() is not None and parallel.world()[1] == world
    stats = dict(solver.last_solve_stats)
    vm = solver.von_Mises(u).vector().get_local()
    if rank == 0:
        result = dict(x=u.vector().get_local(), von_mises=vm, iterations=stats["iterations"],
                      amg_decomposition=np.array(stats.get("amg_decomposition", "")))
    parallel.barrier()
    parallel.finalize()
else:
    raise SystemExit("unknown case %r" % case)

if rank == 0:
    np.savez(out_path, **result)
