"""The margin arithmetic of the witness sweep on the GPU, word for word (flooder_wit_probe_f32, csrc/flood_wit.hip).

The probe runs phase 1 of wit_sweep_kernel - Region::fill, c_max, bin_scale, the gather box, Excess - with the sweep's
own code and writes out every number its pruning rests on: the Region words, the Excess members, per point excess and
bin, per sample its coordinates, slack and limit(slack, k / bin_scale).  Inputs are those of
tests/test_wit_sorted_stage_cpu.py: the replica's simplices (slivers, flat, axis-parallel, offset by 1e3) and its
points, those exactly on bin boundaries included.

1. Every output word equals the replica's (tests/wit_reference.py).  Zeros are compared as zeros: the maxima and
   minima in these expressions do not order +0 and -0.
2. The CPU test's statement with the DEVICE's numbers: every point of a bin k >= 1 has a squared distance - replayed in
   the arithmetic of the pair loops - strictly above the device's limit of that bin, for every sample.

Runs on a real MI355X only (-m gpu)."""
import itertools

import numpy as np
import pytest
import torch

from flooder_amd import _native
from wit_reference import NBIN, Region, f32, pair_d2, points, simplices

pytestmark = pytest.mark.gpu

PER_EDGE, N_GUARD, GUARD = 5, 64, -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    _native.load()
    return torch.device("cuda:0")


def _weights(k1):
    """the lattice of Region.samples"""
    n = PER_EDGE - 1
    rows = [c for c in itertools.product(range(n + 1), repeat=k1) if sum(c) == n]
    return (np.array(rows, f32) / f32(n)).astype(f32)


def _probe(dim, verts, cmax_frac, pts, pt_off, weights, dev):
    """the probe's output, cut into its parts (numpy)"""
    lib = _native.load()
    S, P, R = verts.shape[0], pts.shape[0], weights.shape[0]
    W, E, C = (dim + 1) * dim + 4 * (dim + 1) + 3 * dim + 2, 2 * dim + 3 * (dim + 1), 2 + 2 * dim
    sizes = [24 * S, W * S, E * S, C * S, P, (dim + 1) * R * S, (NBIN + 1) * R * S]
    out = torch.full((sum(sizes) + N_GUARD,), GUARD, dtype=torch.float32, device=dev)
    bins = torch.full((P + N_GUARD,), -7, dtype=torch.int32, device=dev)
    args = [torch.as_tensor(a, device=dev).contiguous() for a in (verts, pts, pt_off, weights)]
    _native.check(lib.flooder_wit_probe_f32(_native.ptr(args[0]), dim, S, float(cmax_frac), _native.ptr(args[1]),
                                            _native.ptr(args[2]), P, _native.ptr(args[3]), R, _native.ptr(out),
                                            _native.ptr(bins), _native.current_stream_ptr(dev)), "flooder_wit_probe_f32")
    torch.cuda.synchronize()
    out, bins = out.cpu().numpy(), bins.cpu().numpy()
    assert (out[-N_GUARD:] == f32(GUARD)).all() and (bins[-N_GUARD:] == -7).all(), "written behind the output"
    assert not (bins[:P] == -7).any()
    parts, at = [], 0
    for n in sizes:
        parts.append(out[at:at + n])
        at += n
    planes, region, excess, scalars, pt_excess, samples, limits = parts
    return dict(region=region.reshape(S, W), excess=excess.reshape(S, E), scalars=scalars.reshape(S, C),
                pt_excess=pt_excess, bins=bins[:P], samples=samples.reshape(S, R, dim + 1),
                limits=limits.reshape(S, R, NBIN + 1))


def _same(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))


@pytest.mark.parametrize("cmax_frac", [0.6, 0.15])
@pytest.mark.parametrize("dim", [2, 3])
def test_probe_words_equal_the_replica_and_bins_lie_beyond_their_limits(dim, cmax_frac, dev):
    named = simplices(dim)
    regions, pts = [], []
    for si, (name, vs) in enumerate(named):
        rg = Region(vs, cmax_frac)
        regions.append(rg)
        pts.append(points(rg, np.random.default_rng(1000 * dim + si)))
    pt_off = np.concatenate([[0], np.cumsum([len(x) for x in pts])]).astype(np.int64)
    weights = _weights(dim + 1)
    got = _probe(dim, np.stack([vs for _, vs in named]), cmax_frac, np.concatenate(pts), pt_off, weights, dev)
    ks = np.arange(NBIN + 1, dtype=f32)
    wrong, on_boundary, pairs, not_beyond = [], 0, 0, []
    for si, ((name, vs), rg, x) in enumerate(zip(named, regions, pts)):
        # ---- 1. the words
        want_region = np.concatenate(
            [np.concatenate([rg.pn[f], [rg.po[f], rg.ps[f], rg.slo[f], rg.shi[f]]]) for f in range(dim + 1)]
            + [np.array([rg.org[k], rg.blo[k], rg.bhi[k]]) for k in range(dim)] + [[rg.sext, rg.epsb]]).astype(f32)
        want_excess = np.concatenate([np.array([rg.blo_e[k], rg.bhi_e[k]]) for k in range(dim)]
                                     + [np.array([rg.slo_t[f], rg.shi_t[f], rg.inv_den[f]]) for f in range(dim + 1)]).astype(f32)
        qlo, qhi = (rg.blo_e - rg.c_max).astype(f32), (rg.bhi_e + rg.c_max).astype(f32)
        want_scalars = np.concatenate([[rg.c_max, rg.bin_scale], np.stack([qlo, qhi], 1).ravel()]).astype(f32)
        e = rg.excess(x)
        with np.errstate(over="ignore", invalid="ignore"):
            eb = (e * rg.bin_scale).astype(f32)
        want_bins = np.where(eb < f32(NBIN), eb, f32(NBIN)).astype(np.int32)
        p = rg.samples(PER_EDGE)
        dl = rg.slack(p)
        want_samples = np.concatenate([p, dl[:, None]], 1)
        want_limits = Region.limit(dl[:, None], (ks / rg.bin_scale).astype(f32)[None, :])
        a, b = pt_off[si], pt_off[si + 1]
        for what, g, w in (("Region", got["region"][si], want_region), ("Excess", got["excess"][si], want_excess),
                           ("c_max, bin_scale, gather box", got["scalars"][si], want_scalars),
                           ("excess of the points", got["pt_excess"][a:b], e), ("samples and slacks", got["samples"][si], want_samples),
                           ("limits", got["limits"][si], want_limits)):
            n_bad = int((~_same(g, w)).sum())
            if n_bad:
                wrong.append(f"{name}: {what}: {n_bad} of {np.size(w)} words")
        if not np.array_equal(got["bins"][a:b], want_bins):
            wrong.append(f"{name}: bins: {int((got['bins'][a:b] != want_bins).sum())} of {len(want_bins)}")
        # ---- 2. the statement, with the device's numbers
        k = got["bins"][a:b]
        keep = (k >= 1) & (k < NBIN)
        deb = (got["pt_excess"][a:b] * got["scalars"][si, 1]).astype(f32)
        on_boundary += int((deb[keep] == k[keep]).sum())
        d2 = pair_d2(got["samples"][si][:, :dim].copy(), x[keep])
        lim = got["limits"][si][:, k[keep]]
        pairs += d2.size
        n_bad = int((~(d2 > lim)).sum())
        if n_bad:
            not_beyond.append((name, n_bad))
    print(f"dim {dim}, c_max {cmax_frac} of the extent: {pt_off[-1]} points, {pairs} (sample, point) pairs of the bins >= 1, "
          f"{on_boundary} points exactly on a bin boundary; words wrong: {wrong[:6]}; not beyond the limit: {not_beyond[:6]}")
    assert pairs > 100_000 and on_boundary > 50
    assert not wrong, wrong[:12]
    assert not not_beyond, not_beyond[:12]
