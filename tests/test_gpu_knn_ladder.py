"""Every step of the slot ladder of the k-nearest family on the device.  A lane keeps its k best in K registers, K = k
rounded up to 2, 4, 8, 16 or 32, one kernel instantiation each; the ``KS`` of the other k-nearest tests never sit on both
sides of the steps 4 | 5 and 16 | 17.  Here k runs over both sides of every step, and for both statistics the words of
``flooder_sweep_knn_f32``, ``flooder_sweep_knn_sorted_f32``, ``flooder_knn_ids_sorted_f32`` (``out_bits``),
``flooder_sweep_knn_profile_f32`` (column (k, stat)) and ``flooder_knn_merge_f32`` over the lists of two half-clouds are
the float64 brute force's, bit for bit: integer coordinates on a narrow lattice, where every d2 is exact in float32 and
most values tie."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import grad_reference as gr
import test_gpu_knn_sorted as tks
from helpers import smallest32

pytestmark = pytest.mark.gpu

DEV = tks.DEV
KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)
PPE = 5                      # lattice(5, 4): R = 70 rows, one full tile of 64 samples and a partial one
N_SIMPLICES = 3              # 210 samples: three full tiles of the sorted order and a partial one
# name -> (dim, points, half-width of the integer lattice): two tree levels with a partial last leaf; one level in 8-D
CLOUDS = {"3d": (3, 1030, 8), "8d": (8, 300, 2)}


@functools.lru_cache(maxsize=None)
def _cloud(name):
    dim, n, r = CLOUDS[name]
    assert n % 16 != 0 and tks._levels(n) == (2 if name == "3d" else 1)
    rng = np.random.default_rng(900 + dim)
    P = rng.integers(-r, r + 1, size=(n, dim))
    V = rng.integers(-r, r + 1, size=(N_SIMPLICES, 5, dim))
    W = gr.lattice(PPE, 4)
    assert W.shape == (70, 5)
    gr.assert_exact_inputs(P, V.reshape(-1, dim), PPE)
    tp = torch.as_tensor(P, dtype=torch.float32, device=DEV)
    t_v = torch.as_tensor(V, dtype=torch.float32, device=DEV).contiguous()
    t_w = W.to(torch.float32).to(DEV).contiguous()
    samples = torch.einsum("rk,skd->srd", W.to(DEV), torch.as_tensor(V, dtype=torch.float64, device=DEV))
    small = smallest32(tp.double(), samples.reshape(-1, dim))
    assert (small[:, 1:] == small[:, :-1]).mean() > 0.25          # the ties are there
    lib = _native.load()
    c = dict(dim=dim, n=n, points=tp, index=core.PointIndex(tp), verts=t_v, weights=t_w, k1=5, R=70, n_s=N_SIMPLICES,
             small=small)
    c["order"] = core._sorted_sample_order(lib, tks._stream(), c["index"], t_v, t_w, None, None,
                                           int(lib.flooder_sample_key_bits(dim)))
    c["halves"] = [core.PointIndex(tp[: n // 2].contiguous()), core.PointIndex(tp[n // 2:].contiguous())]
    return c


def _lattice_fields(c, index):
    return dict(pts_sorted=index.pts, n_pts=index.n, dim=c["dim"], k1=c["k1"], nodes=index.nodes, verts=c["verts"],
                weights=c["weights"], R=c["R"], n_simplices=c["n_s"],
                queue=torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV))


def _profile(c, index, columns):
    """The (len(columns), S, R) planes of ``flooder_sweep_knn_profile_f32`` over the points of ``index``."""
    planes = torch.full((len(columns), c["n_s"], c["R"]), -1, dtype=torch.int32, device=DEV)
    blk = _native.KnnProfile(columns, out_bits=planes, **_lattice_fields(c, index))
    _native.check(_native.load().flooder_sweep_knn_profile_f32(ctypes.byref(blk), tks._stream()),
                  "flooder_sweep_knn_profile_f32")
    return planes


def _ids_bits(c, k, stat):
    N = c["n_s"] * c["R"]
    ids = torch.full((N, k), -1, dtype=torch.int32, device=DEV)
    bits = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    blk = _native.KnnIds(k=k, stat=stat, out_bits=bits, sample_order=c["order"], order=c["index"].order32, out_ids=ids,
                         **_lattice_fields(c, c["index"]))
    _native.check(_native.load().flooder_knn_ids_sorted_f32(ctypes.byref(blk), tks._stream()),
                  "flooder_knn_ids_sorted_f32")
    return bits


def _merged(c, lists, k, stat):
    N = c["n_s"] * c["R"]
    out = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    blk = _native.KnnMerge(lists=lists, n_cells=N, n_lists=int(lists.shape[0]), k=k, stat=stat, out_bits=out)
    _native.check(_native.load().flooder_knn_merge_f32(ctypes.byref(blk), tks._stream()), "flooder_knn_merge_f32")
    return out


def _words(t):
    return t.cpu().numpy().view(np.uint32).reshape(-1)


def test_the_ks_sit_on_both_sides_of_every_step():
    slots = lambda k: next(K for K in (2, 4, 8, 16, 32) if k <= K)   # noqa: E731
    for below in (2, 4, 8, 16):
        assert below in KS and below + 1 in KS and slots(below) == below and slots(below + 1) == 2 * below
    assert 1 in KS and 32 in KS and max(KS) <= min(c[1] for c in CLOUDS.values()) // 2


@pytest.mark.parametrize("name", list(CLOUDS))
def test_every_entry_writes_the_brute_force_words_at_every_k(name):
    c = _cloud(name)
    for k in KS:
        planes = _profile(c, c["index"], [(k, 0), (k, 1)])
        lists = torch.stack([_profile(c, half, [(t, 0) for t in range(1, k + 1)]) for half in c["halves"]]).contiguous()
        for stat in (0, 1):
            want = tks._expected(c["small"], k, stat)
            got = {"per-simplex": tks._sweep(c, k, stat),
                   "sorted": tks._sweep(c, k, stat, c["order"]),
                   "ids": _words(_ids_bits(c, k, stat)),
                   "profile": _words(planes[stat]),
                   "merge": _words(_merged(c, lists, k, stat))}
            for entry, words in got.items():
                assert np.array_equal(words, want), (name, entry, k, tks.STATS[stat], np.argwhere(words != want)[:5].ravel())
