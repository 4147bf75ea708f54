"""Bit check of two libmfea.so builds over the boundary forms.

Each library runs in its own child process (MFEA_LIB=...) and takes the same
sequence on the planar and the 3-D golden mesh: 3 grip forms (the tensile
test, two directions with a z component, a grip field) x 3 load forms (none,
dead, proportional), each through mfea_solve with Jacobi and block Jacobi,
a GAMG solve after an assembly, two GAMG steps (the fused assembly RHS, then
the kept hierarchy) with amg_start and step_graph off and on, and, where the
load mode allows it, one mfea_event.  A record holds status, iterations, an
md5 of U, the force, grip_work and load_work; the parent compares the records
of the libraries and writes them out once.

    python tools/bc_form_bitcheck.py --libs abso/libmfea_parent.so mycelium-fea-project_amd/libmfea.so \\
        --out profiles/bc_form/bitcheck_parent_vs_new.json
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESHES = {"planar": ("sim_20251117_175809", 1.5), "sim3d": ("sim_20251115_135507", 0.5)}
AMP, MAX_STRAIN = 0.05, 0.018
JACOBI, BJACOBI, GAMG = 0, 1, 2


def child():
    sys.path.insert(0, os.path.join(REPO, "mycelium-fea-project_amd"))
    sys.path.insert(0, os.path.join(REPO, "oracle"))
    import numpy as np
    import pandas as pd

    import fea_oracle as fo
    import fea_solver as fs
    from mfea import Engine, fields, loads, make_opts

    def opts(pc):
        return make_opts(precond=pc, rtol=1e-9, max_it=200000)

    eng = Engine(0)
    eng.set_option("amg_rebuild_rent", 0)
    eng.set_material(fs.E_mod, fs.A, fs.I)
    out = {}

    def record(st, force=None, **more):
        U = eng.displacement()
        gw = eng.grip_work()
        r = {"status": st.status, "iters": st.iters, "U_md5": hashlib.md5(np.ascontiguousarray(U).tobytes()).hexdigest(),
             "grip_work": [float.hex(gw[0]), float.hex(gw[1])], "load_work": float.hex(eng.load_work())}
        if force is not None:
            r["force"] = float.hex(force)
        r.update(more)
        return r

    for mname, (mesh, tol) in MESHES.items():
        d = os.path.join(REPO, "tests", "golden", "meshes", mesh)
        nodes, elems = pd.read_csv(os.path.join(d, "nodes.csv")), pd.read_csv(os.path.join(d, "elements.csv"))
        xyz, e2n = nodes[["x", "y", "z"]].values, elems[["n1", "n2"]].values
        top, bot = fo.grip_nodes(xyz, nodes["node_id"].values, tol)
        n = len(xyz)
        grip = np.zeros(n, bool)
        grip[top] = grip[bot] = True
        free = np.flatnonzero(~grip)
        pick = free[np.linspace(0, len(free) - 1, 7).astype(int)[1:-1]]
        f_dead = loads.point(n, pick, (2.0e-8, -4.0e-8, 1.5e-8)) + loads.self_weight(xyz, e2n, 1.0e-8, (0.0, -1.0, 0.0))
        grips = {
            "tensile": dict(motion=((0.0, 1.0, 0.0), (0.0, 1.0, 0.0)), field=None),
            "vec_z": dict(motion=((0.48, 0.6, 0.64), (0.0, 0.8, -0.6)), field=None),
            "field": dict(motion=((0.0, 1.0, 0.0), (0.0, 1.0, 0.0)),
                          field=fields.rigid_rotation(xyz, top, (0.3, 0.0, 0.954)) +
                          fields.uniform(n, bot, (0.0, 0.8, -0.6))),
        }
        lds = {"none": (None, "dead"), "dead": (f_dead, "dead"), "proportional": (f_dead / AMP, "proportional")}
        eng.set_mesh(xyz, e2n)
        eng.set_bc(top, bot)
        for gname, g in grips.items():
            for lname, (f, mode) in lds.items():
                eng.set_active(None)
                eng.set_grip_motion(*g["motion"])
                eng.set_grip_field(g["field"])
                eng.set_node_loads(f, mode)
                rec = []
                for pc, tag in ((JACOBI, "solve_jacobi"), (BJACOBI, "solve_bjacobi"), (GAMG, "solve_gamg")):
                    eng.assemble()
                    rec.append(record(eng.solve(AMP, -AMP, opts(pc)), path=tag))
                for start in (0, 1):
                    for graph in (0, 1):
                        eng.set_option("amg_start", start)
                        eng.set_option("step_graph", graph)
                        eng.set_active(None)
                        for k in range(2):
                            force, n_act, st = eng.step(AMP, -AMP, opts(GAMG), 1.0)
                            rec.append(record(st, force, path="step%d_start%d_graph%d" % (k, start, graph),
                                              n_active=n_act))
                if lname != "dead":
                    eng.set_active(None)
                    lam, force1, n_failed, n_act, st = eng.event(AMP, -AMP, opts(GAMG), MAX_STRAIN, lam_max=1e6)
                    rec.append(record(st, force1, path="event", lam=float.hex(lam), n_failed=n_failed,
                                      n_active=n_act))
                out["%s/%s/%s" % (mname, gname, lname)] = rec
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child()
        return
    got = []
    for lib in a.libs:
        env = dict(os.environ, MFEA_LIB=os.path.abspath(lib))
        r = subprocess.run([sys.executable, __file__, "--child"], env=env, capture_output=True, text=True,
                           timeout=420)
        if r.returncode != 0:
            print(json.dumps({"lib": lib, "rc": r.returncode, "err": r.stderr[-3000:]}), flush=True)
            sys.exit(r.returncode if r.returncode > 0 else 1)
        got.append(json.loads(r.stdout.strip().splitlines()[-1]))
    same = got[0] == got[1]
    differ = sorted(k for k in got[0] if got[0][k] != got[1].get(k))
    res = {"identical": same, "libs": [os.path.basename(x) for x in a.libs], "combinations": len(got[0]),
           "records_per_lib": sum(len(v) for v in got[0].values()), "differ": differ,
           "records": got[0] if same else {"a": got[0], "b": got[1]}}
    text = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(json.dumps({k: res[k] for k in ("identical", "libs", "combinations", "records_per_lib", "differ")}))
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
