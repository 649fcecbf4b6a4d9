"""Operands on which the split-bf16 convolutions have no rounding at all, so that their results must equal fp64 `conv2d` bit for bit (test_conv_exact.py
checks the generator on the CPU, test_gpu_conv_exact.py the kernels).

The kernels (csrc/smd_conv_mfma.hip, smd_conv_wgrad.hip, smd_conv_stem.hip; their shared stages: csrc/smd_conv_mfma_dev.h) split every fp32 operand into
three bf16 pieces, a = a0 + a1 + a2, and keep the six products a_i b_j with i + j <= 2.  A PIECE-BUILT value is  s (n0 + n1 2^-10 + n2 2^-20) 2^e  with s = +-1 and n0, n1, n2 in {1, 2, 3}: its round-to-nearest-even split
returns exactly s n0 2^e, s n1 2^(e-10), s n2 2^(e-20) (all pieces share the sign: 1 - 3 2^-10 re-splits differently, the bf16 ulp halves below 1, and
`from_pieces` refuses it).  Three operand FAMILIES make the products the scheme drops (a1 b2, a2 b1, a2 b2) exactly zero while every kept product is
exercised by one of them; `lead` = n0 only, `two` = n0 + n1 2^-10, `full` = all three:

    A: a full, b lead   (a0 b0, a1 b0, a2 b0)        B: a lead, b full   (a0 b0, a0 b1, a0 b2)        C: a two, b two   (a0 b0, a0 b1, a1 b0, a1 b1)

A product of two such values spans at most 24 bits, so it is an fp32 number, and in the IMPULSE layouts below every output element is one product: whatever
order the kernel adds in, it adds zeros.  The DENSE family has small integers everywhere: every partial sum is an integer below 2^24."""
import torch

KEPT = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))    # (piece of a, piece of b), smallest first: `prod_a` / `prod_b` of csrc/smd_split_dev.h
FAMILIES = {'A': ('full', 'lead'), 'B': ('lead', 'full'), 'C': ('two', 'two')}
# exponents of (activation x, weight, dL/dy): all 0, and a real step's magnitudes (dL/dy around 1e-7, large weights): exactness must not depend on them
SCALES = {'unit': (0, 0, 0), 'spread': (0, 20, -30)}

# (B, C, CO, h, w) of the 3x3 forms and (B, C, H, W) of the stem: the smallest shapes that reach each kernel form (what each reaches: the comments at
# the same shapes in test_gpu_parity.py, test_gpu_encoder_conv.py, test_gpu_conv_band_tiles.py, test_gpu_stem_conv.py)
PADDED = [(2, 16, 32, 5, 7), (1, 32, 32, 33, 65), (2, 48, 64, 9, 70), (3, 160, 64, 6, 20), (2, 64, 128, 4, 20), (2, 32, 64, 4, 1), (2, 64, 64, 1, 49),
          (2, 128, 64, 10, 47), (2, 16, 16, 7, 70), (2, 32, 16, 9, 33), (1, 16, 16, 2, 2)]
SAME = [(2, 64, 64, 1, 1), (3, 64, 64, 5, 7), (5, 32, 64, 1, 49), (2, 64, 64, 3, 1), (2, 64, 32, 9, 3), (2, 128, 64, 10, 47), (1, 64, 64, 11, 49),
        (1, 64, 64, 13, 100), (1, 512, 64, 4, 20), (5, 512, 512, 3, 5)]
STEM = [(2, 3, 1, 1), (2, 3, 5, 7), (2, 6, 13, 101), (3, 6, 37, 64), (1, 3, 37, 64)]
BF16 = [(2, 16, 16, 7, 70), (2, 64, 64, 9, 70), (2, 96, 32, 13, 100), (2, 32, 16, 9, 33)]
# `conv_two_tiles`: 256 tiles of 64 x 4 pixels in the forward (126 x 62) AND in the data gradient (the padded 128 x 64), neither on row bands (conv_shape)
TWO_TILES = (8, 64, 64, 126, 62)


def split3(x):
    """fp32 -> its three bf16 pieces (as fp32), round to nearest even, the way `split_pair` of csrc/smd_split_dev.h forms them."""
    p0 = x.to(torch.bfloat16).float()
    r = x - p0
    p1 = r.to(torch.bfloat16).float()
    r = r - p1
    return p0, p1, r.to(torch.bfloat16).float()


def from_pieces(p0, p1, p2, e=0):
    """(p0 + p1 2^-10 + p2 2^-20) 2^e as fp32, from integer tensors of SIGNED pieces.  Asserts that fp32 holds the fp64 sum and that the three-way split of
    the value returns exactly the pieces it was built from."""
    p = [t.double() for t in (p0, p1, p2)]
    want = (p[0]*2.0**e, p[1]*2.0**(e - 10), p[2]*2.0**(e - 20))
    x64 = want[0] + want[1] + want[2]
    x = x64.float()
    assert torch.equal(x.double(), x64), 'the value is not an fp32 number'
    for k, (g, w) in enumerate(zip(split3(x), want)):
        assert torch.equal(g.double(), w), f'piece {k} of the three-way bf16 split is not the piece the value was built from'
    return x


class Pieces:
    """Integer pieces of a tensor of values; `at(e)` -> the fp32 tensor at exponent e (checked by `from_pieces`)."""
    def __init__(self, p0, p1, p2): self.p = (p0, p1, p2)
    def at(self, e=0): return from_pieces(*self.p, e)
    @property
    def shape(self): return tuple(self.p[0].shape)


def draw(shape, kind, gen) -> Pieces:
    """Random pieces.  full / two / lead: piece-built values (see the module text); int1, int2: dense integers in {-1 .. 1}, {-2 .. 2}; int15: nonzero
    integers of magnitude up to 15 (one bf16 piece each, for bfloat16 tensors)."""
    ri = lambda lo, hi: torch.randint(lo, hi + 1, shape, generator=gen)
    zero = torch.zeros(shape, dtype=torch.int64)
    if kind in ('int1', 'int2'): return Pieces(ri(-1, 1) if kind == 'int1' else ri(-2, 2), zero, zero)
    r = ri(0, 2*3*3*3 - 1)                                      # one draw per element: sign and the three digits
    s, n0, n1, n2 = (r % 2)*2 - 1, (r//2) % 3 + 1, (r//6) % 3 + 1, (r//18) % 3 + 1
    if kind == 'int15': return Pieces(s*ri(1, 15), zero, zero)
    if kind not in ('full', 'two', 'lead'): raise ValueError(kind)
    return Pieces(s*n0, s*n1 if kind != 'lead' else zero, s*n2 if kind == 'full' else zero)


# ---- layouts: which elements of a (B, C, H, W) tensor are nonzero in one run (flat indices) --------------------------------------------------------

def lattice_phases(shape, step):
    """Impulses on a lattice of spacing `step` in y and x (3 for the 3x3 kernels, 7 for the stride-2 7x7 one: no output sees two sites), ONE channel per
    site, the channel cycling over the sites.  One phase per lattice offset, so that every (sample, y, x) carries an impulse in some phase, then further
    phases with the channel assignment carried on until every channel has carried one.  -> list of flat index tensors."""
    B, C, H, W = shape
    offsets = [(oy, ox) for oy in range(min(step, H)) for ox in range(min(step, W))]
    phases, start, k = [], 0, 0
    while k < len(offsets) or start < C:
        oy, ox = offsets[k % len(offsets)]
        b, y, x = (t.reshape(-1) for t in torch.meshgrid(torch.arange(B), torch.arange(oy, H, step), torch.arange(ox, W, step), indexing='ij'))
        ch = (start + torch.arange(b.numel())) % C
        phases.append(((b*C + ch)*H + y)*W + x)
        start += b.numel(); k += 1
    return phases


def one_per_channel(shape, runs, gen):
    """The weight gradient's activation: exactly ONE nonzero element per channel over the whole batch, so that g_w[co, c, tap] is one product with a dense
    dL/dy.  The positions are drawn from borders, corners, the columns and rows where pixel tiles of 32 / 64 x 4 / 8 and row bands end, and the middle,
    over all samples; `runs` rotations.  -> list of flat index tensors."""
    B, C, H, W = shape
    ys = sorted({v for v in (0, 1, 2, 3, 4, 7, 8, H//2, H - 3, H - 2, H - 1) if 0 <= v < H})
    xs = sorted({v for v in (0, 1, 2, 31, 32, 33, 63, 64, 65, W//2, W - 3, W - 2, W - 1) if 0 <= v < W})
    b, y, x = (t.reshape(-1) for t in torch.meshgrid(torch.arange(B), torch.tensor(ys), torch.tensor(xs), indexing='ij'))
    order = torch.randperm(b.numel(), generator=gen)
    c = torch.arange(C)
    out = []
    for r in range(runs):
        sel = order[(c + r*C) % order.numel()]
        out.append(((b[sel]*C + c)*H + y[sel])*W + x[sel])
    return out


def keep_only(values, idx):
    """`values` with everything but the flat positions `idx` set to zero."""
    out = torch.zeros_like(values)
    idx = idx.to(values.device)
    out.view(-1)[idx] = values.reshape(-1)[idx]
    return out


def impulse_stack(values, phases):
    """(number of phases, *values.shape): `values` kept at each phase's positions only."""
    return torch.stack([keep_only(values, idx) for idx in phases])


# ---- the scheme in plain torch (the CPU test's model of the kernels) -----------------------------------------------------------------------------------

def emulate(a, b, op, products=KEPT, order='split'):
    """The split-bf16 scheme: split both fp32 operands, form `op(a_i, b_j)` (a bilinear operator: a product, a convolution) for the `products` kept, each
    as an fp32 tensor, and add them in fp32.  order 'split': the kernels' two accumulators (everything but the last product, smallest first, then the last
    plus that sum); 'descending' / 'ascending': one accumulator, largest / smallest first."""
    pa, pb = split3(a), split3(b)
    terms = [op(pa[i], pb[j]) for i, j in products]
    assert all(t.dtype == torch.float32 for t in terms)
    if order == 'split':
        lo = torch.zeros_like(terms[0])
        for t in terms[:-1]: lo = lo + t
        return terms[-1] + lo
    acc = torch.zeros_like(terms[0])
    for t in (reversed(terms) if order == 'descending' else terms): acc = acc + t
    return acc


def first_difference(got, ref, names):
    """None where the tensors are equal, else 'names = index: got g, expected r' for the first differing element and the number that differ."""
    if got.shape != ref.shape: return f'shape {tuple(got.shape)} instead of {tuple(ref.shape)}'
    ne = got != ref
    n = int(ne.sum())
    if n == 0: return None
    flat = int(ne.reshape(-1).to(torch.uint8).argmax())
    idx = []
    for d in reversed(got.shape): idx.append(flat % d); flat //= d
    idx = tuple(reversed(idx))
    return (f'{n} of {got.numel()} elements differ, first at ({", ".join(names)}) = {idx}: got {got[idx].item()!r} ({got[idx].double().item().hex()}), '
            f'expected {ref[idx].item()!r} ({ref[idx].double().item().hex()})')
