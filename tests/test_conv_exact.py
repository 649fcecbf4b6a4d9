"""The exact-arithmetic operands of conv_exact.py can see what they are meant to see — checked without a GPU on a plain-torch model of the split-bf16
scheme (`conv_exact.emulate`): with all six products every family at both scales equals fp64 bit for bit in three summation orders; with any one product
removed, or a third-order product computed twice in place of another, essentially every element of the family that exercises it differs; and the layouts
make every output element a single product while covering every input position and channel."""
import pytest
import torch
import torch.nn.functional as TF

import conv_exact as X

ORDERS = ('split', 'descending', 'ascending')
N = 200_000
THIRD = [(2, 0), (1, 1), (0, 2)]


def _gen(seed): return torch.Generator().manual_seed(seed)


def _pairs(family, scale, seed=0):
    """N operand pairs (a, b) of a family; at 'spread' a takes dL/dy's exponent and b the weights'."""
    ka, kb = X.FAMILIES[family]
    _, ew, eg = X.SCALES[scale]
    gen = _gen(seed)
    return X.draw((N,), ka, gen).at(eg), X.draw((N,), kb, gen).at(ew)


def _differing(products, family, scale):
    a, b = _pairs(family, scale)
    exact = a.double()*b.double()
    return min(((X.emulate(a, b, torch.mul, products, o).double() != exact).double().mean().item()) for o in ORDERS)


@pytest.mark.parametrize('scale', list(X.SCALES))
@pytest.mark.parametrize('family', list(X.FAMILIES))
def test_six_products_reproduce_fp64(family, scale):
    a, b = _pairs(family, scale)
    exact = a.double()*b.double()
    assert torch.equal(exact.float().double(), exact)             # the product itself is an fp32 number
    for order in ORDERS: assert torch.equal(X.emulate(a, b, torch.mul, order=order).double(), exact), order
    pa, pb = X.split3(a), X.split3(b)                            # what the scheme drops is exactly zero
    for i, j in ((1, 2), (2, 1), (2, 2)): assert not (pa[i]*pb[j]).any()


@pytest.mark.parametrize('scale', list(X.SCALES))
@pytest.mark.parametrize('removed', X.KEPT)
def test_a_removed_product_is_seen(removed, scale):
    products = [p for p in X.KEPT if p != removed]
    seen = {f: _differing(products, f, scale) for f in X.FAMILIES}
    print(f'a{removed[0]} b{removed[1]} removed, {scale}: share of elements that differ', seen)
    assert max(seen.values()) >= 0.99, seen


@pytest.mark.parametrize('scale', list(X.SCALES))
@pytest.mark.parametrize('slot,twice', [(s, t) for s in THIRD for t in THIRD if s != t] + [((1, 0), (0, 1)), ((0, 1), (1, 0))])
def test_a_product_computed_twice_in_place_of_another_is_seen(slot, twice, scale):
    """Every third-order product replaced by a second copy of each other third-order product (a2 b0 <-> a0 b2 are the mirror swaps; a1 b1 is its own
    mirror, so it is replaced by either neighbour), and the second-order mirror swaps."""
    products = [twice if p == slot else p for p in X.KEPT]
    seen = {f: _differing(products, f, scale) for f in X.FAMILIES}
    print(f'a{twice[0]} b{twice[1]} twice in place of a{slot[0]} b{slot[1]}, {scale}: share of elements that differ', seen)
    assert max(seen.values()) >= 0.99, seen


def test_mixed_signs_are_refused():
    one = torch.ones(4, dtype=torch.int64)
    X.from_pieces(one, 3*one, 2*one)
    X.from_pieces(-one, -3*one, -2*one, -30)
    with pytest.raises(AssertionError): X.from_pieces(one, -3*one, 0*one)       # 1 - 3 2^-10: the bf16 ulp halves below 1, the split moves
    with pytest.raises(AssertionError): X.from_pieces(5*one, 300*one, one)      # pieces that overlap


def test_dense_and_bf16_kinds():
    gen = _gen(1)
    for kind, lo, hi in (('int1', -1, 1), ('int2', -2, 2), ('int15', -15, 15)):
        v = X.draw((4096,), kind, gen).at(-30 if kind == 'int15' else 20)*2.0**(30 if kind == 'int15' else -20)
        assert v.min() == lo and v.max() == hi and torch.equal(v, v.round())
        assert torch.equal(v.to(torch.bfloat16).float(), v)
        if kind == 'int15': assert (v != 0).all()


# ---- the layouts ---------------------------------------------------------------------------------------------------------------------------------------
CONVS = {'padded': (3, dict()), 'same': (3, dict(padding=1)), 'stem': (7, dict(stride=2, padding=3))}


@pytest.mark.parametrize('form,shape', [('padded', (2, 16, 7, 9)), ('padded', (1, 40, 4, 4)), ('same', (3, 32, 5, 7)), ('same', (2, 64, 1, 1)), ('same', (2, 8, 3, 1)),
                                        ('stem', (2, 3, 5, 7)), ('stem', (2, 6, 13, 29)), ('stem', (2, 3, 1, 1))])
def test_lattice_phases_cover_everything_one_product_per_output(form, shape):
    k, kw = CONVS[form]
    B, C, H, W = shape
    phases = X.lattice_phases(shape, k)
    ones = torch.ones(shape, dtype=torch.float64)
    stack = X.impulse_stack(ones, phases)
    assert len(phases) >= min(k, H)*min(k, W)
    assert (stack.sum(2) <= 1).all()                              # one channel per site
    assert (stack.sum((0, 2)) >= 1).all()                         # every (sample, y, x) carries an impulse in some phase
    assert (stack.sum((0, 1, 3, 4)) >= 1).all()                   # every channel has carried one
    hits = TF.conv2d(stack.flatten(0, 1), torch.ones(1, C, k, k, dtype=torch.float64), **kw)
    assert hits.max() == 1                                        # no output element sees two impulses
    if form == 'padded': assert hits.min() == 1                   # ... and with no zero padding every one sees exactly one


def test_one_per_channel():
    shape = (3, 40, 12, 70)
    runs = X.one_per_channel(shape, 4, _gen(2))
    ones = torch.ones(shape)
    seen = set()
    for idx in runs:
        m = X.keep_only(ones, idx)
        assert (m.sum((0, 2, 3)) == 1).all()
        seen |= set(idx.tolist())
    assert len(seen) == 4*40                                       # the rotations move every channel's element
    pos = torch.stack([X.keep_only(ones, idx) for idx in runs]).sum((0, 2))
    assert (pos.sum((1, 2)) > 0).all() and pos[:, 0].any() and pos[:, -1].any() and pos[:, :, 0].any() and pos[:, :, -1].any() and pos[:, :, 63:65].any()


@pytest.mark.parametrize('scale', list(X.SCALES))
@pytest.mark.parametrize('family', list(X.FAMILIES))
def test_emulated_convolution_is_exact_on_the_layouts(family, scale):
    """A whole small convolution through the model: output (impulse x, dense weight), input gradient (impulse dL/dy, dense weight) and weight gradient (one
    element of x per channel, dense dL/dy) equal fp64 in every order; with a2 b0 / a0 b2 / a1 b1 removed the family that exercises it loses at least 99 % of
    its nonzero elements."""
    B, C, CO, h, w = 2, 16, 32, 5, 7
    ka, kb = X.FAMILIES[family]
    ex, ew, eg = X.SCALES[scale]
    gen = _gen(3)
    x, wt = X.draw((B, C, h + 2, w + 2), ka, gen).at(ex), X.draw((CO, C, 3, 3), kb, gen).at(ew)
    gy_a, gy_b = X.draw((B, CO, h, w), ka, gen).at(eg), X.draw((B, CO, h, w), kb, gen).at(eg)
    xs = X.impulse_stack(x, X.lattice_phases(x.shape, 3)).flatten(0, 1)
    gs = X.impulse_stack(gy_a, X.lattice_phases(gy_a.shape, 3)).flatten(0, 1)
    xo = X.keep_only(x, X.one_per_channel(x.shape, 1, gen)[0])

    def f32(t):
        assert torch.equal(t.float().double(), t)
        return t.float()
    ops = {'output': (xs, wt, lambda a, b: f32(TF.conv2d(a.double(), b.double()))),
           'input gradient': (gs, wt, lambda a, b: f32(TF.conv_transpose2d(a.double(), b.double()))),
           'weight gradient': (xo, gy_b, lambda a, b: f32(TF.conv2d(a.double().transpose(0, 1), b.double().transpose(0, 1)).transpose(0, 1)))}
    exercised = {'A': (2, 0), 'B': (0, 2), 'C': (1, 1)}[family]
    for name, (a, b, op) in ops.items():
        exact = op(a, b).double()
        assert (exact != 0).double().mean() > (0.99 if name == "output" else 0.2)
        for order in ORDERS: assert torch.equal(X.emulate(a, b, op, order=order).double(), exact), (name, order)
        broken = X.emulate(a, b, op, [p for p in X.KEPT if p != exercised]).double()
        assert ((broken != exact) & (exact != 0)).sum() >= 0.99*(exact != 0).sum(), name


def test_dense_integer_sums_stay_below_2_24():
    """|v| <= 2: a sum of n products is at most 4 n — every partial sum of every operator at every shape the GPU test runs is an integer fp32 holds."""
    for B, C, CO, h, w in X.PADDED + X.SAME + [X.TWO_TILES]:
        assert 4*9*max(C, CO) < 2**24 and 4*B*(h + 2)*(w + 2) < 2**24
    for B, C, H, W in X.STEM:
        assert 4*49*C < 2**24 and 4*B*H*W < 2**24
    for B, C, CO, h, w in X.BF16: assert B*(h + 2)*(w + 2) < 2**24     # |v| <= 1, the fp32 weight gradient
