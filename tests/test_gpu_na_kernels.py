"""The Neighbourhood Algorithm's cell-walk kernels (csrc/sx_na.hip), driven one generation at a time through the C ABI
(tests/_na_abi.py) on model stores made up here, at the sizes whole runs do not reach: more than 64 walks (the draw
kernel's second workgroup), more than 16 384 models (the cap of sx_na_blocks: the grid-stride loop of the axis kernel),
rows of up to 1 030 axes (three levels of the in-thread replica of numpy's pairwise summation), fixed axes at either end
and side by side, and degenerate cells (NaN and infinite walls, both clamps, no wall at all).

The reference of a walk is oracle.engine.na_walk, which the goldens pin to the reference's mutation() bit for bit; every
operation involved is + - * /, a comparison, fmax or fmin, so every comparison here is bit for bit too.  Every case runs
twice: with NaN in the padding of the store and of the cell distances (columns >= M), and with numbers from [0, 1) there,
which a kernel that reads past M would take for models."""
import collections

import numpy as np
import pytest

import _na_abi
from oracle.engine import na_walk
from oracle.streams import PhiloxStream

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Bit for bit: NaN equals the same NaN, 0.0 does not equal -0.0."""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def store(rs, M, n, grid):
    """Models in the unit cube: on a grid of 1 / 16 (equal coordinates, duplicate models and exact ties between walls
    are the rule there) or random doubles."""
    return rs.randint(0, 17, (M, n)) / 16.0 if grid else rs.random_sample((M, n))


def centres(rs, M, P):
    """Model 0, model M - 1, one model twice and a model of the last partial block of 256, then random ones.  Three walks
    hold them as 0, M - 1, M - 1 (the last model lies in the last block); a single walk starts at M - 1."""
    last = 256 * ((M - 1) // 256)
    if P == 1:
        return np.array([M - 1])
    if P < 5:
        return np.array([0, M - 1, M - 1, M // 2][:P])
    want = [0, M - 1, M // 2, M // 2, last + (M - 1 - last) // 2]
    return np.array(want + rs.randint(0, M, P - len(want)).tolist())


class Walls(collections.Counter):
    """na_walk's probe: what kinds of wall and of interval the numpy walk met."""

    def __call__(self, j, lim, xj):
        below, above = lim <= xj, lim >= xj
        self["nan"] += int(np.isnan(lim).sum())
        self["+inf"] += int((lim == np.inf).sum())
        self["-inf"] += int((lim == -np.inf).sum())
        self["none below"] += int(not below.any())
        self["none above"] += int(not above.any())
        self["low clamped"] += int(below.any() and lim[below].max() < 0.0)
        self["high clamped"] += int(above.any() and lim[above].min() > 1.0)


def check(models, kidx, u, free, seed):
    """The device's generation against na_walk, and everything it must leave alone.  Returns the wall counts."""
    M, n = models.shape
    P = len(kidx)
    free = np.asarray(free, dtype=bool)
    cap = M + P + 37
    seen = Walls()
    ref = np.array([na_walk(models, int(k), u[i], free, probe=seen) for i, k in enumerate(kidx)])
    assert _na_abi.blocks(M) == min(-(-M // 256), 64)
    from stochopy_amd import _lib

    assert _lib.lib().sx_na_blocks(M) == _na_abi.blocks(M)
    rs = np.random.RandomState(seed)
    runs = [_na_abi.walks(models, cap, kidx, u, free, pad) for pad in (np.nan, rs.random_sample)]
    for out in runs:
        for i in range(P):
            assert same(out["X"][i], ref[i]), f"walk {i} from model {kidx[i]}: {out['X'][i]} != {ref[i]}"
        assert same(out["XT"][:, :M], models.T), "the stored models changed"
        assert same(out["XT"][:, M:M + P], ref.T), "the committed columns are not the new samples"
        assert (out["XT"][~free, M:M + P] == 0.0).all()
        assert same(out["XT"][:, M + P:], out["XT0"][:, M + P:]), "the store's padding past M + P changed"
        assert same(out["d2"][:, M:], out["d20"][:, M:]), "the cell distances' padding changed"
        assert same(out["d2_begin"][:, M:], out["d20"][:, M:]), "sx_na_begin wrote cell distances past M"
        for i, k in enumerate(kidx):
            x, others = models[k], np.delete(models, k, axis=0)
            want = ((others[:, 1:] - x[1:]) ** 2).sum(axis=1)  # the oracle's own expression (na_walk)
            assert same(np.delete(out["d2_begin"][i, :M], k), want), f"walk {i}: d2 after sx_na_begin"
    a, b = runs
    assert same(a["X"], b["X"]) and same(a["XT"][:, :M + P], b["XT"][:, :M + P])
    assert same(a["d2_begin"][:, :M], b["d2_begin"][:, :M]) and same(a["d2"][:, :M], b["d2"][:, :M])
    return seen


def plant_neighbours(models, kidx, step):
    """The models a shortened sweep would miss -- the last one, and the first of a thread's second and third trip (64
    workgroups of 256 threads) -- become the nearest neighbours of three cell centres, `step` away along axis 0: a walk
    that does not see them draws between other walls there.  (Among tens of thousands of models one that is left out seldom
    bounds any of five cells by itself.)"""
    M = len(models)
    probes = [m for m in dict.fromkeys((M - 1, 16384, 32768)) if m < M]
    for probe, centre in zip(probes, (kidx[2], kidx[0], kidx[4])):
        if probe != centre:
            models[probe] = models[centre]
            models[probe, 0] += step if models[centre, 0] < 0.5 else -step


def generation(P, M, n, grid, seed, fixed=(), plant=False):
    rs = np.random.RandomState(seed)
    models = store(rs, M, n, grid)
    free = np.ones(n, dtype=bool)
    free[list(fixed)] = False
    if fixed:  # what a real store holds: the bound itself in the first generation, 0.0 in every sample of a walk
        models[:, ~free] = 0.0
        models[:P, ~free] = 1.5
    kidx = centres(rs, M, P)
    if plant:  # half a grid step, or well inside the distance between random neighbours (about 0.55 * M ** (-1 / 3))
        plant_neighbours(models, kidx, 1.0 / 32 if grid else 1.0 / 1024)
    return check(models, kidx, rs.random_sample((P, n)), free, seed + 1)


FLAVOURS = pytest.mark.parametrize("grid", [True, False], ids=["grid", "random"])


@FLAVOURS
@pytest.mark.parametrize("M", [2, 255, 256, 257, 768, 769, 16384, 16385, 17157, 40000])
def test_model_count(M, grid):
    """One block, the edges of one, three and four blocks, the last size without a stride (64 blocks), the first with one,
    a thread's second trip ending inside a block, and two to three trips.  The last model and the first models of the
    second and third trip are planted next to cell centres, so that each of them is a wall."""
    generation(5, M, 3, grid, 1000 + M, plant=True)


@FLAVOURS
@pytest.mark.parametrize("n", [1, 2, 8, 9, 129, 130, 258, 1030])
def test_row_length(n, grid):
    """n - 1 terms in the initial cell distances: none (no recurrence either), one, 7 and 8 (the leaf's two forms), 128
    and 129 (the largest leaf, the first split), 257 (a split whose right half splits again) and 1 029 (three levels).  The order of the sum shows in the random flavour
    only: on the grid every term is a multiple of 1 / 256 and every partial sum exact."""
    generation(3, 300, n, grid, 2000 + n)


@FLAVOURS
@pytest.mark.parametrize("P", [1, 64, 65, 130])
def test_walk_count(P, grid):
    """The draw kernel serves 64 walks per workgroup: one, a full workgroup, one walk in the second, a third workgroup."""
    generation(P, 300, 3, grid, 3000 + P)


@FLAVOURS
@pytest.mark.parametrize("fixed", [(0,), (4,), (1, 2), (0, 4), (0, 1, 2, 3), (1, 2, 3, 4)], ids=str)
def test_fixed_axes(fixed, grid):
    """A fixed axis first, last, next to another one, at both ends, and all but one: the deferred update of the cell
    distances names the previous FREE axis jp and its right neighbour jp + 1, which may be fixed."""
    generation(6, 300, 5, grid, 4000 + sum(2 ** j for j in fixed), fixed)


def _copies(rs, models, kidx, u):
    models[150] = models[299] = models[17]  # three copies of a centre: 0 / 0 walls
    return ("nan",)


def _flat_axis(rs, models, kidx, u):
    models[:, 1] = 0.5  # every model has the centre's coordinate: division by zero on that axis
    u[:, 0] = 0.0       # ... with the walker ON a wall of axis 0, so that the sign of d1 - d2 goes either way
    return ("+inf", "-inf", "none above")


def _face(rs, models, kidx, u):
    models[:, 0] *= 1.0 / 512  # crowded at the face x_0 = 0: most walls along axis 0 lie outside the unit cube
    kidx[4], kidx[5] = models[:, 0].argmin(), models[:, 0].argmax()  # (model M - 1 stays, in the last block of 256)
    return ("low clamped", "high clamped", "none below", "none above")


@pytest.mark.parametrize("degenerate", [_copies, _flat_axis, _face], ids=lambda f: f.__name__[1:])
def test_degenerate_cells(degenerate):
    """NaN walls (both comparisons must skip them), infinite walls, both clamps, and no wall on one side or the other.
    What each store must provoke is counted in the numpy walk, so that a case cannot quietly stop being degenerate;
    together the three cover all seven kinds."""
    P, M, n = 6, 300, 3
    rs = np.random.RandomState(5004)  # (chosen in the numpy walk: four +inf walls, not one)
    models, kidx, u = store(rs, M, n, False), centres(rs, M, P), rs.random_sample((P, n))
    required = degenerate(rs, models, kidx, u)
    seen = check(models, kidx, u, np.ones(n, dtype=bool), 5005)
    print(degenerate.__name__, dict(seen))
    for kind in required:
        assert seen[kind] >= 1, (kind, dict(seen))


def test_degenerate_cells_cover_every_kind():
    """The three stores of test_degenerate_cells name all seven kinds between them (no GPU work)."""
    rs = np.random.RandomState(0)
    named = set()
    for degenerate in (_copies, _flat_axis, _face):
        named.update(degenerate(rs, store(rs, 300, 3, False), centres(rs, 300, 6), rs.random_sample((6, 3))))
    assert named == {"nan", "+inf", "-inf", "none below", "none above", "low clamped", "high clamped"}


SEED = 0x5DEECE66D1234567  # wider than 32 bits: both key words matter


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 32, 33, 64, 65, 128, 129, 257, 1030])
def test_uniforms(n):
    """sx_na_uniforms against the oracle's Philox block: 16, 32 and 64 lanes per row and the steps around them, one to 300
    rows (more than one workgroup at every n), a generation counter with the top bit set."""
    stream = PhiloxStream(SEED)
    for P in (1, 3, 300):
        for gen in (2, 2 ** 31 + 5):
            want = stream.na_uniforms(gen, P, n, np.ones(n, dtype=bool))
            got = _na_abi.uniforms(SEED, gen, P, n)
            assert same(got, want), (P, gen)
            assert ((want >= 0.0) & (want < 1.0)).all()
