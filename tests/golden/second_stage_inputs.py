"""The two forwards whose loss goes through the one-block fp64 second stage (`launch_sum_partials_f64`, csrc/smd_misc.hip): the fused masked image
reconstruction and the fused feature-metric reconstruction, n = 2, in-kernel noise of a fixed seed: at 17 x 23, S = 2, b = 2 (12 and 10 block sums: one wave of the second
stage) and at 65 x 100, S = 4, b = 2 | b = 8 (288 and 272 block sums: past the 256 threads, so the strided loop takes a second step and all four waves add in their order).  Shared by
make_golden_second_stage.py (which records the losses' bit patterns) and tests/test_gpu_second_stage.py (which asserts them)."""
import torch

N, SEED = 2, 7
SHAPES = {'small': dict(H=17, W=23, S=2, B=2, FB=2), 'large': dict(H=65, W=100, S=4, B=2, FB=8)}      # FB: the feature case's batch


def mask_inputs(case='small'):
    H, W, S, B = (SHAPES[case][k] for k in ('H', 'W', 'S', 'B'))
    from slowtv_monodepth_amd.synthetic import kitti_K
    g = torch.Generator().manual_seed(20261 + 10*(case == 'large'))
    Ts = torch.eye(4).repeat(N, B, 1, 1); Ts[..., :3, 3] = 0.05*torch.randn(N, B, 3, generator=g)
    imgs = torch.rand(B, 3, H, W, generator=g)
    return dict(depth=0.5 + 5*torch.rand(S, B, H, W, generator=g), mask=0.3*torch.randn(S, B, N, H, W, generator=g), imgs=imgs,
                supp=0.6*imgs[None] + 0.4*torch.rand(N, B, 3, H, W, generator=g), Ts=Ts, K=kitti_K(B, H, W))


def feat_inputs(case='small', C=6):
    H, W, B = (SHAPES[case][k] for k in ('H', 'W', 'FB'))
    hf, wf = (H + 3)//4, (W + 3)//4
    from slowtv_monodepth_amd.synthetic import kitti_K
    g = torch.Generator().manual_seed(20262 + 10*(case == 'large'))
    feats = torch.randn(B, C, hf, wf, generator=g)
    Ts = torch.eye(4).repeat(N, B, 1, 1); Ts[..., :3, 3] = 0.05*torch.randn(N, B, 3, generator=g)
    return dict(depth=1 + 9*torch.rand(B, 1, H, W, generator=g), feats=feats, supp=0.5*torch.randn(N, B, C, hf, wf, generator=g) + 0.5*feats[None], Ts=Ts, K=kitti_K(B, H, W))


def loss_bits(mask_in, feat_in):
    """-> {'mask_recon': int, 'feat_recon': int}: the float32 losses' bit patterns, of the operands given (CPU tensors; run on cuda:0)."""
    from slowtv_monodepth_amd import featrecon, maskrecon
    m = {k: v.cuda() for k, v in mask_in.items()}
    f = {k: v.cuda() for k, v in feat_in.items()}
    with torch.no_grad():
        lm = maskrecon.mask_recon_loss(m['depth'], m['mask'], m['imgs'], m['supp'], m['Ts'], m['K'], loss_name='ssim', use_min=True, use_automask=True,
                                       mask_name='uncertainty', seed=SEED, want_warp=False)[0]
        lf = featrecon.feat_recon_loss(f['depth'], f['feats'], f['supp'], f['Ts'], f['K'], loss_name='l2', use_min=True, use_automask=True, seed=SEED)[0]
    return {'mask_recon': int(lm.view(torch.int32).item()), 'feat_recon': int(lf.view(torch.int32).item())}
