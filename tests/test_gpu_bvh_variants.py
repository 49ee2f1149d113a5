"""Every instantiation of the tree sweep (csrc/flood_bvh.hip, sweep_bvh_kernel<DIM, KS, LB>) word for word against the
float64 brute force over all points, on the exact cases of ``variant_cases``:

* ``flooder_sweep_bvh_f32`` under option "bvh_ks" 1, 2, 4 and 8 (tiles of 64, 128, 256 and 512 samples against weight
  matrices of 63 to 513 rows), under "bvh_grid" 1, 3 and 65536 and with the transposed refine always / never taken;
* ``flooder_sweep_bvh_items_f32`` called directly: the full list, a partial list, seeded words, the static deal and
  the queue, tiles split over 1, 16 and 64 waves, leaves fetched one and four at a time, and the budgeted two-pass form
  on both sides of the kernel's "at most 2048 items" rule.

Every output buffer is prefilled and carries guard words behind it.  Runs on a real MI355X only (-m gpu)."""
import numpy as np
import pytest
import torch

from flooder_amd import _native, core

import variant_cases as vc
from variant_cases import INF_BITS, UNWRITTEN, kernel_case, options, same_words

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MINE = vc.SET_BY["test_gpu_bvh_variants"]


def _stream():
    return _native.current_stream_ptr(DEV)


def _queue():
    return torch.zeros(core.QUEUE_WORDS, dtype=torch.int32, device=DEV)


def _tree_sweep(c, what):
    """flooder_sweep_bvh_f32 under the options in force: (the (S * R) words, the counters)."""
    words = c.n_s * c.R
    out, stats = vc.guarded(words, UNWRITTEN, DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    _native.check(_native.load().flooder_sweep_bvh_f32(
        _native.ptr(c.index.pts), c.index.n, c.dim, _native.ptr(c.index.nodes), _native.ptr(c.verts), _native.ptr(c.weights),
        c.k1, c.R, c.n_s, _native.ptr(_queue()), _native.ptr(out), _native.ptr(stats), _stream()), "flooder_sweep_bvh_f32")
    got, s = vc.read_guarded(out, words, what), stats.cpu().numpy()
    same_words(got, c.want, what)
    assert s[0] > 0 and s[1] > 0 and s[2] > 0, (what, s.tolist())      # leaves evaluated, leaves tested, nodes expanded
    return s


def test_cases_cover_what_they_must():
    assert {c[0] for c in vc.CASES} == {2, 3, 6}
    for dim in (2, 3, 6):
        mine = [c for c in vc.CASES if c[0] == dim]
        assert {vc.levels(c[1]) for c in mine} == {1, 2, 3} and {c[2] for c in mine} == {True, False}
        assert sum(c[4] == vc.ALL_R for c in mine) == 1
    assert all(c[1] % 16 != 0 and 8 <= c[3] <= 30 for c in vc.CASES)
    # a tile of 64 * KS samples, KS = 1, 2, 4, 8: a matrix that fills its last tile and one with a single row in it
    assert all(any(R % (64 * ks) == 0 for R in vc.ALL_R) and any(R % (64 * ks) == 1 for R in vc.ALL_R) for ks in MINE["bvh_ks"])


@pytest.mark.parametrize("dim,n,R", vc.CASE_R, ids=vc.CASE_R_IDS)
def test_tree_sweep_words_under_every_ks(dim, n, R):
    c = kernel_case(dim, n, R)
    for ks in MINE["bvh_ks"]:
        with options(bvh_ks=ks):
            _tree_sweep(c, ("flooder_sweep_bvh_f32", "bvh_ks", ks))


@pytest.mark.parametrize("dim,n,R", vc.THREE_LEVEL, ids=vc.THREE_LEVEL_IDS)
def test_tree_sweep_words_under_every_grid(dim, n, R):
    """One workgroup (four waves drain all queue shards), three, and far more workgroups than items."""
    c = kernel_case(dim, n, R)
    for grid in MINE["bvh_grid"]:
        with options(bvh_grid=grid):
            _tree_sweep(c, ("flooder_sweep_bvh_f32", "bvh_grid", grid))


def test_tree_sweep_words_with_and_without_the_refine():
    """"bvh_refine_pct" 1: the transposed refine wherever a leaf group has a candidate; INT_MAX: never.  Same words; the
    counters differ on at least one case, so both sides ran."""
    differ = 0
    for dim, n, R in vc.THREE_LEVEL:
        c = kernel_case(dim, n, R)
        seen = []
        for pct in MINE["bvh_refine_pct"]:
            with options(bvh_refine_pct=pct):
                seen.append(_tree_sweep(c, ("flooder_sweep_bvh_f32", "bvh_refine_pct", pct))[:3].tolist())
        print(dim, n, R, "refine always / never:", seen)
        differ += seen[0] != seen[1]
    assert differ > 0, "the counters never differ: one side of the refine did not run"


# ------------------------------------------------------------------------------------------------ the work-list sweep
def _tiles(c):
    return (c.R + 63) // 64


def _items_sweep(c, items, out, n_s=None, verts=None, budget=0, what=""):
    """flooder_sweep_bvh_items_f32 on the list `items` (simplex * tiles + tile), starting from the words in `out`
    (guarded).  budget > 0: returns the second list the call wrote, else None."""
    n_s = c.n_s if n_s is None else n_s
    verts = c.verts if verts is None else verts
    lst = torch.as_tensor(np.asarray(items, dtype=np.int32), device=DEV)
    cnt = torch.tensor([lst.numel()], dtype=torch.int32, device=DEV)
    stats = torch.zeros(8, dtype=torch.int64, device=DEV)
    list2 = vc.guarded(lst.numel(), 0, DEV) if budget > 0 else None
    count2 = torch.zeros(1, dtype=torch.int32, device=DEV) if budget > 0 else None
    _native.check(_native.load().flooder_sweep_bvh_items_f32(
        _native.ptr(c.index.pts), c.index.n, c.dim, _native.ptr(c.index.nodes), _native.ptr(verts), _native.ptr(c.weights),
        c.k1, c.R, n_s, _native.ptr(lst), _native.ptr(cnt), _native.ptr(_queue()), _native.ptr(out), budget,
        _native.ptr(list2), _native.ptr(count2), _native.ptr(stats), _stream()), "flooder_sweep_bvh_items_f32")
    torch.cuda.synchronize()
    if budget == 0:
        return None
    n2 = int(count2.item())
    assert 0 <= n2 <= lst.numel(), (what, n2)
    return vc.read_guarded(list2, lst.numel(), what)[:n2].astype(np.int64)


def _tile_mask(c, items, n_s=None):
    """(S * R) bools: the words of the listed tiles"""
    n_s = c.n_s if n_s is None else n_s
    mask = np.zeros((n_s, _tiles(c) * 64), dtype=bool)
    items = np.asarray(items, dtype=np.int64)
    for s, t in zip(items // _tiles(c), items % _tiles(c)):
        mask[s, t * 64:(t + 1) * 64] = True
    return mask[:, :c.R].reshape(-1)


@pytest.mark.parametrize("dim,n,R", vc.CASE_R, ids=vc.CASE_R_IDS)
def test_items_full_list_split_and_batched(dim, n, R):
    """Every (simplex, tile) item listed, seeds +inf: tiles whole (bvh_subs 1), split over 16 waves, and over 64 -
    asked for, and picked by the kernel itself on the lists of at most 64 items -, leaves one and four at a time."""
    c = kernel_case(dim, n, R)
    items = np.arange(c.n_s * _tiles(c))
    for subs in (1, 16, 64):
        for batch in (1, 4):
            with options(bvh_subs=subs, bvh_leaf_batch=batch):
                out = vc.guarded(c.n_s * R, INF_BITS, DEV)
                _items_sweep(c, items, out)
                same_words(vc.read_guarded(out, c.n_s * R, (subs, batch)), c.want, ("items", "subs", subs, "batch", batch))


ITEM_CASES = [(dim, n, R) for dim, n, R in vc.CASE_R if R in vc.FEW_R]
ITEM_IDS = [f"{dim}d-{n}-R{R}" for dim, n, R in ITEM_CASES]


@pytest.mark.parametrize("dim,n,R", ITEM_CASES, ids=ITEM_IDS)
@pytest.mark.parametrize("batch", [1, 4])
def test_items_partial_list(dim, n, R, batch):
    """Every third item listed: its words are the brute force's, every other word is still its prefill."""
    c = kernel_case(dim, n, R)
    items = np.arange(c.n_s * _tiles(c))[::3]
    listed = _tile_mask(c, items)
    assert listed.any() and not listed.all()
    fill = np.where(listed, INF_BITS, UNWRITTEN).astype(np.int32)
    out = vc.guarded(c.n_s * R, torch.as_tensor(fill, device=DEV), DEV)
    with options(bvh_leaf_batch=batch):
        _items_sweep(c, items, out)
    got = vc.read_guarded(out, c.n_s * R, "partial list")
    same_words(got[listed], c.want[listed], "listed tiles")
    assert (got[~listed].view(np.int32) == UNWRITTEN).all(), "a word of a tile that is not listed was written"


@pytest.mark.parametrize("dim,n,R", ITEM_CASES, ids=ITEM_IDS)
@pytest.mark.parametrize("batch", [1, 4])
def test_items_seeded(dim, n, R, batch):
    """The words the call starts from: a third the exact minimum, a third the distance to one fixed point of the cloud
    (a valid upper bound), a third +inf.  All exact afterwards - a seed at the minimum stays what it is."""
    c = kernel_case(dim, n, R)
    kind = np.random.default_rng(R + n).integers(0, 3, size=c.n_s * R)
    seed = np.where(kind == 0, c.want, np.where(kind == 1, _distance_words(_samples(c, c.verts), torch.as_tensor(c.base.P[0], dtype=torch.float64, device=DEV)), np.uint32(INF_BITS))).astype(np.uint32)
    assert (seed.view(np.float32) >= c.want.view(np.float32)).all() and (seed != c.want).mean() > 0.5
    items = np.arange(c.n_s * _tiles(c))
    for grid in (None, 1):    # the static deal or the queue by the list's length, and the queue for certain
        out = vc.guarded(c.n_s * R, torch.as_tensor(seed.view(np.int32), device=DEV), DEV)
        with options(bvh_leaf_batch=batch, **({} if grid is None else {"bvh_grid": grid})):
            assert grid is None or len(items) > 4 * grid
            _items_sweep(c, items, out)
        same_words(vc.read_guarded(out, c.n_s * R, "seeded"), c.want, ("seeded", "bvh_grid", grid))


def _samples(c, verts):
    """(S * R, dim) float64 samples of `verts` under the case's weights (exact)"""
    return torch.einsum("rk,skd->srd", c.base.W[:c.R].to(DEV), verts.double()).reshape(-1, c.dim)


def _distance_words(q, point):
    """float32 words of the squared distance of every row of q to `point` (asserted exact)"""
    d2 = ((q - point) ** 2).sum(dim=1).cpu().numpy()
    f = d2.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), d2)
    return f.view(np.uint32)


def _members(c, q, words):
    """True where the word is the squared distance of its sample to SOME point of the cloud (float64, all points)."""
    P = torch.as_tensor(c.base.P, dtype=torch.float64, device=DEV)
    w = torch.as_tensor(words.view(np.float32).astype(np.float64), device=DEV)
    per = max(1, (1 << 26) // P.shape[0])
    hit = []
    for a in range(0, q.shape[0], per):
        d2 = (q[a:a + per, 0:1] - P[:, 0].unsqueeze(0)) ** 2
        for k in range(1, c.dim):
            d2 += (q[a:a + per, k:k + 1] - P[:, k].unsqueeze(0)) ** 2
        hit.append((d2 == w[a:a + per, None]).any(dim=1))
    return torch.cat(hit).cpu().numpy()


# (dim, n, R, copies of the simplices, budget): 8 to 30 simplices of up to 9 tiles are a list of at most 2048 items -
# the kernel's rule makes the budget 1 there -; thirty copies of them are one of more.  The first copy is then
# replaced by simplices whose vertices are all ONE point of the cloud: every sample of theirs is that point, its minimum
# is 0 by construction, and a search that goes to the nearest leaf first is over after one box test per tree level and
# one leaf - below the budget of 12 -, while a tile of 64 rows drawn from all over a wide simplex meets more leaves
# than that.
BUDGET_CASES = [(dim, n, R, 1, 50) for dim, n, R in ITEM_CASES] + [(2, 1025, 513, 30, 12), (3, 70_001, 513, 30, 12),
                                                                   (6, 1025, 513, 30, 12)]


@pytest.mark.parametrize("dim,n,R,reps,budget", BUDGET_CASES, ids=[f"{c[0]}d-{c[1]}-R{c[2]}-x{c[3]}" for c in BUDGET_CASES])
def test_items_budgeted_two_passes(dim, n, R, reps, budget):
    """budget > 0: a wave gives a tile up after that many box tests, stores the minima it has and appends the tile to
    list2; a second call on list2 without a budget finishes them.  The words start as the distance to one fixed point.
    After the first call every word is at least the brute force and the distance to a real point, list2 holds listed
    items only and none twice; after the second all words are exact."""
    c = kernel_case(dim, n, R)
    n_s = c.n_s * reps
    verts = c.verts.repeat(reps, 1, 1).contiguous()
    want = np.tile(c.want, reps)
    if reps > 1:
        verts[:c.n_s] = c.index.pts[:c.n_s, None, :dim].expand(-1, c.k1, -1)
        want[:c.n_s * R] = 0
    items = np.arange(n_s * _tiles(c))
    items = items if reps > 1 else items[items % 5 != 3]
    assert (len(items) > 2048) == (reps > 1)
    listed = _tile_mask(c, items, n_s)
    q = _samples(c, verts)
    seed = _distance_words(q, torch.as_tensor(c.base.P[1], dtype=torch.float64, device=DEV))
    assert (seed.view(np.float32) >= want.view(np.float32)).all()
    out = vc.guarded(n_s * R, torch.as_tensor(seed.view(np.int32), device=DEV), DEV)
    list2 = _items_sweep(c, items, out, n_s=n_s, verts=verts, budget=budget, what="budgeted pass")
    first = vc.read_guarded(out, n_s * R, "budgeted pass")
    print(f"{dim}-D n {n} R {R} x{reps}: {len(items)} items, {len(list2)} given up; exact after the first pass: "
          f"{(first[listed] == want[listed]).mean():.1%}")
    assert len(set(list2.tolist())) == len(list2) and set(list2.tolist()) <= set(items.tolist())
    if reps == 1:
        assert len(list2) == len(items), "a short list hands every tile to the second pass"
    else:
        assert 0 < len(list2) < len(items), "the budget gave up none or all of the tiles: one side of it did not run"
    assert (first.view(np.float32) >= want.view(np.float32)).all(), "a word below the true minimum"
    assert (first[~listed] == seed[~listed]).all(), "a word of a tile that is not listed was written"
    assert _members(c, q, first).all(), "a word that is the distance to no point of the cloud"
    done = _tile_mask(c, np.setdiff1d(items, list2), n_s)
    same_words(first[done], want[done], "tiles the first pass did not give up")
    _items_sweep(c, list2, out, n_s=n_s, verts=verts, what="second pass")
    second = vc.read_guarded(out, n_s * R, "second pass")
    same_words(second[listed], want[listed], "after the second pass")
    assert (second[~listed] == seed[~listed]).all()
