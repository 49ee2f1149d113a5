"""Shared helpers of the parity tests."""
import glob
import os
import subprocess
import sys
import textwrap

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Parity bar (BASELINE.json north_star): filtration values within 1e-5 relative in fp32.
# The absolute floor covers the exact zeros (vertices: a landmark is its own nearest point) and the
# input quantisation: a float32 sample coordinate of magnitude c carries ulp(c) ~ 1.2e-7*c, which no
# float32 implementation can undercut; COORD_ULPS of it are allowed (observed errors stay below 1 ulp).
RTOL = 1e-5
COORD_ULPS = 2.0


def get_options(lib, *names):
    """{name: current value} of these options of libflooder_hip.so (names as bytes): what a test records before it
    changes one, and puts back with ``set_options`` afterwards - no copies of the defaults in the tests."""
    import ctypes

    found = {}
    for name in names:
        value = ctypes.c_int()
        assert lib.flooder_get_option(name, ctypes.byref(value)) == 0, name
        found[name] = value.value
    return found


def set_options(lib, values):
    for name, value in values.items():
        assert lib.flooder_set_option(name, int(value)) == 0, name


def tolerances(points):
    scale = float(np.abs(np.asarray(points)).max())
    return RTOL, COORD_ULPS * np.finfo(np.float32).eps * max(scale, 1e-30)


def assert_baseline_gate(got, ref, points, what=""):
    """BASELINE.md section 3's parity gate, as written there (and as ``bench.py`` applies it): relative error
    ``|got - ref| / max(|ref|, 1e-6 * diameter) <= 1e-5`` - NO absolute ulp term.  The diameter is taken as the
    longest side of the cloud's bounding box (never more than the true diameter: the stricter reading).  Used on the
    BASELINE configurations at full size, where the HIP path has 60x margin; the small goldens keep the ulp term of
    ``assert_close_filtration`` (two of them differ from the reference's CPU branch by float32 matmul order)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    P = np.asarray(points)
    floor = 1e-6 * float((P.max(axis=0) - P.min(axis=0)).max())
    fin = np.isfinite(ref)
    assert (np.isfinite(got) == fin).all(), f"{what}: infinities differ"
    rel = np.abs(got[fin] - ref[fin]) / np.maximum(np.abs(ref[fin]), floor)
    assert rel.size == 0 or rel.max() <= RTOL, (
        f"{what}: BASELINE gate (rel 1e-5, floor 1e-6 x diameter) failed: worst {rel.max():.3e} "
        f"on {int((rel > RTOL).sum())}/{rel.size} values")
    return float(rel.max()) if rel.size else 0.0


def assert_close_filtration(got, ref, points, what="", strict=False):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if strict:
        assert_baseline_gate(got, ref, points, what)
    rtol, atol = tolerances(points)
    both_inf = np.isinf(got) & np.isinf(ref)
    both_nan = np.isnan(got) & np.isnan(ref)
    err = np.where(both_inf | both_nan, 0.0, np.abs(got - ref))
    bound = atol + rtol * np.abs(np.where(np.isfinite(ref), ref, 0.0))
    bad = ~(err <= bound)
    assert not bad.any(), (
        f"{what}: {int(bad.sum())}/{bad.size} values off; worst abs err {np.nanmax(err):.3e} "
        f"(rtol {rtol:g}, atol {atol:.3e})")
    return float(np.nanmax(err)) if err.size else 0.0


def e2e_cases():
    return sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLDEN, "e2e_*.npz")))


def load_e2e(name):
    z = np.load(os.path.join(GOLDEN, f"e2e_{name}.npz"))
    ppe, nr, md = int(z["points_per_edge"]), int(z["num_rand"]), int(z["max_dimension"])
    kwargs = dict(points_per_edge=None if ppe < 0 else ppe, num_rand=None if nr < 0 else nr,
                  max_dimension=None if md < 0 else md)
    keys = [tuple(int(v) for v in row if v >= 0) for row in z["simplices"]]
    return z, kwargs, keys


def dict_values(fc, keys):
    return np.array([fc[k] for k in keys], dtype=np.float64)


def kdtree_face_values(tree, landmarks, simplices, points_per_edge, d, chunk_queries=4_000_000, dtype=np.float32):
    """Reference values of all dimension-``d`` simplices (rows of landmark ids): the reference's CPU computation
    (``core.py:188, 197-199, 251-257``) - barycentric lattice of ``points_per_edge`` per edge on the simplex itself,
    nearest neighbour of every sample by ``tree.query`` on all host cores, maximum over the samples.  Queried in
    chunks so that the (queries, dim) float64 copy scipy makes stays below a few hundred MB."""
    from oracle import flood_oracle as fo

    w, _, _ = fo.generate_grid(points_per_edge, d, dtype)
    R = w.shape[0]
    per = max(1, chunk_queries // R)
    out = np.empty(len(simplices), dtype=np.float64)
    for b in range(0, len(simplices), per):
        verts = landmarks[simplices[b:b + per]]
        samples = np.matmul(w[None], verts).astype(dtype)
        dist, _ = tree.query(samples, workers=-1)
        out[b:b + per] = dist.max(axis=1)
    return out


def assert_tree_matches_kdtree(st, points, landmarks, points_per_edge, top, what, pick_top=None, lower=True,
                               strict=False):
    """Every simplex of dimension ``top`` of the simplex tree ``st`` (or the rows ``pick_top`` of that table), and
    - ``lower`` - every simplex of the dimensions below, against the kd-tree over ALL ``points``: a face of a swept
    simplex carries the maximum over ITS OWN lattice samples (the zero weights of the parent's lattice rows contribute
    exact zeros), so each table is checked with the lattice of its own dimension.  ``strict``: BASELINE.md's gate
    (``assert_baseline_gate``) on top of the usual one.  Returns the number of values checked."""
    from scipy.spatial import cKDTree

    tree = cKDTree(points, balanced_tree=False, compact_nodes=False)
    n = 0
    for d in range(top, 0, -1):
        rows = st.simplices_of_dimension(d)
        vals = st.filtrations_of_dimension(d)
        if d == top and pick_top is not None:
            rows, vals = rows[pick_top], vals[pick_top]
        ref = kdtree_face_values(tree, landmarks, rows, points_per_edge, d, dtype=points.dtype.type)
        assert_close_filtration(vals, ref, points, f"{what}: dimension {d}", strict=strict)
        n += len(rows)
        if not lower:
            break
    return n


def _kdtree_reference(fc, P, L, k, ppe=None, weights_by_dim=None, top=None):
    """{stat: {simplex: value}} of every simplex of the dict ``fc`` from ``cKDTree.query(k=k)`` over all points in
    float64: the samples of the simplex's own lattice (float32 weights and vertices, as the sweep sees them) or of the
    drawn weights, the maximum over them, then the monotone pass over the facets.  Simplices above ``top``
    (``max_dimension``) have no samples of their own: the monotone pass alone gives them their facets' maximum."""
    import itertools

    from scipy.spatial import cKDTree

    from flooder_amd import core

    tree = cKDTree(P.astype(np.float64))
    by_dim = {}
    for key in fc:
        by_dim.setdefault(len(key) - 1, []).append(key)
    ref = {"kth": {}, "dtm": {}}
    for d in sorted(by_dim):
        keys = by_dim[d]
        if top is not None and d > top:
            for stat in ("kth", "dtm"):
                for key in keys:
                    ref[stat][key] = max(ref[stat][face] for face in itertools.combinations(key, d))
            continue
        if weights_by_dim is not None:
            w = weights_by_dim[d].numpy()
        elif d == 0:
            w = np.ones((1, 1), dtype=np.float32)
        else:
            w = core.generate_grid(ppe, d, "cpu", torch.float32)[0].numpy()
        for b in range(0, len(keys), max(1, 2_000_000 // w.shape[0])):
            part = keys[b:b + max(1, 2_000_000 // w.shape[0])]
            verts = L[np.array(part)]
            samples = np.matmul(w[None], verts).astype(np.float32).reshape(-1, P.shape[1])
            dist, _ = tree.query(samples.astype(np.float64), k=k, workers=-1)
            dist = dist.reshape(len(part), w.shape[0], k)
            vals = {"kth": dist[..., -1].max(axis=1), "dtm": np.sqrt((dist ** 2).mean(axis=-1)).max(axis=1)}
            for stat in ("kth", "dtm"):
                for key, v in zip(part, vals[stat].tolist()):
                    for face in itertools.combinations(key, d) if d > 0 else ():
                        v = max(v, ref[stat][face])
                    ref[stat][key] = v
    return ref


def smallest32(P: torch.Tensor, Q: torch.Tensor, chunk_elems: int = 1 << 26) -> np.ndarray:
    """float64 brute force on the device of ``P``: per row of Q the 32 smallest squared distances to ALL rows of P, ascending
    (d2 added axis by axis in float64 - exact on these inputs)."""
    n, dim = P.shape
    per = max(1, chunk_elems // n)
    out = []
    for a in range(0, Q.shape[0], per):
        q = Q[a:a + per]
        d2 = (q[:, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for c in range(1, dim):
            d2 += (q[:, c:c + 1] - P[:, c].unsqueeze(0)) ** 2
        out.append(torch.topk(d2, min(32, n), dim=1, largest=False, sorted=True).values.cpu())
    return torch.cat(out).numpy()


def run_on_mkl_compatible_branch(code, tmp_path):
    """Run ``code`` (which fills the dict ``out`` with numpy arrays) in a fresh CPU-only Python process started with
    ``MKL_CBWR=COMPATIBLE``, and return ``out``.

    torch sends contiguous float32 log / sin / cos to MKL's vector math, and MKL picks its code path by the host CPU:
    the same seeded draws differ in the last bit of a few values from one x86 host to another.  MKL's COMPATIBLE branch
    gives the same bits on every x86 host, and the ``*_mkl_compatible`` goldens are the reference's own outputs on it
    (``oracle/make_goldens.py mkl-compatible``).  MKL reads the setting when it starts, hence the fresh process."""
    path = tmp_path / "mkl_compatible_out.npz"
    script = "import numpy as np\nout = {}\n" + textwrap.dedent(code) + f"\nnp.savez({str(path)!r}, **out)\n"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", script]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, MKL_CBWR="COMPATIBLE"), capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(path)
    return {k: z[k] for k in z.files}


def header_numbers(tmp_path, blocks=None, extra=None):
    """Compile a C program against include/flooder_hip.h with the host C compiler and run it (skip without one) ->
    ``{(C type, "sizeof"): bytes, (C type, field): offset}`` for every field of every ``{C type name: _native class}``
    of ``blocks``, and ``{name: value}`` for every ``{name: C expression}`` of ``extra``."""
    import shutil

    import pytest

    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "flooder_hip.h")}"',
             'int main(void) {']
    for cname, cls in (blocks or {}).items():
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'printf("{name} %lld\\n", (long long)({expr}));' for name, expr in (extra or {}).items()]
    src, exe = tmp_path / "header_numbers.c", tmp_path / "header_numbers"
    src.write_text("\n".join(lines + ['return 0; }']))
    subprocess.run([cc, "-o", str(exe), str(src)], check=True)
    out = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        *key, val = line.split()
        out[key[0] if len(key) == 1 else tuple(key)] = int(val)
    assert len(out) == sum(len(c._fields_) + 1 for c in (blocks or {}).values()) + len(extra or {})
    return out
