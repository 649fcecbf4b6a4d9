"""The cases of tests/golden/viz_reference.npz (made by make_golden_viz.py from the reference's `rgb_from_disp` / `rgb_from_feat`), shared by the generator,
tests/test_viz_host.py and tests/test_gpu_viz.py.  The fixture stores the inputs themselves (they are small), so nothing here has to reproduce a bit."""
import numpy as np

# name, shape, invert
DISP_CASES = [('no_positive_and_single', (2, 1, 5, 7), False), ('nan_neg_const_zeros', (3, 1, 24, 33), False), ('invert_with_zeros', (3, 1, 24, 33), True),
              ('one_row', (1, 1, 1, 3), False)]
# name, shape, comparable components — the solver sklearn's 'auto' runs on each is recorded in the fixture (`feat_solver_k`) and stated in make_golden_viz.py.
# c512_n3 has three samples: two non-zero eigenvalues, so its third component (and third output channel: noise over noise) is not comparable.
FEAT_CASES = [('c3', (2, 3, 4, 5), 3), ('c16', (2, 16, 6, 8), 3), ('c64', (1, 64, 12, 20), 3), ('c512', (1, 512, 3, 5), 3), ('c512_n3', (1, 512, 1, 3), 2)]


def pca_fp64(x: np.ndarray) -> np.ndarray:
    """(b,C,h,w) -> (b,3,h,w) float64: the PCA of viz.py:62-74 in float64 with numpy's `eigh` and sklearn's sign rule (the entry of largest magnitude of each
    component is positive), `proj -= min; proj /= max` per channel."""
    b, C, h, w = x.shape
    X = x.astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, C)
    Xc = X - X.mean(0)
    _, vecs = np.linalg.eigh(Xc.T @ Xc)
    V = vecs[:, [-1, -2, -3]]
    V = V*np.sign(V[np.abs(V).argmax(0), np.arange(3)])
    proj = Xc @ V
    proj -= proj.min(0)
    with np.errstate(invalid='ignore', divide='ignore'): proj /= proj.max(0)
    return proj.reshape(b, h, w, 3).transpose(0, 3, 1, 2)


def leading_eigenvalues(x: np.ndarray) -> np.ndarray:
    b, C, h, w = x.shape
    X = x.astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, C)
    Xc = X - X.mean(0)
    return np.linalg.eigvalsh(Xc.T @ Xc)[::-1][:4]
