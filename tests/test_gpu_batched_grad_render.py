"""Training renders as ONE autograd node per batch of views: ``facade.SurfelRenderer.render_view_all(require_grad=True)``
(the path of every training render of the reference, mapping/gaussian_map.py:94-104) through
``rasterizer.rasterize_batch`` (csrc/torch_binding.cpp: RasterizeBatchFn over ags_forward_batch / ags_backward_batch) and
``facade._FacadePostBatch`` (ags_facade_post_batch / ags_facade_post_backward_batch).  Held to the per-view path it
replaces: same images bit for bit, the same gradients up to the order of the atomic sums."""
import os

import numpy as np
import pytest
import torch

from _scenes import oracle_inputs, room_case

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IMAGES = ("rgb", "normal", "depth", "opacity", "confidence")
# The batch sums its views' per-surfel gradients into one slab with atomics; the per-view path sums them in autograd's
# order.  That order alone moves d_scales (whose per-view terms cancel most) by ~1.1e-5 relative L1 on the 20 k-surfel
# scenes below; 40x larger surfels (the repair scene) by ~3e-5 - there the bound of the per-view repair test applies.
GRAD_TOL = 3e-5
GRAD_TOL_LARGE = 1e-4


@pytest.fixture
def fresh_module():
    """every test starts from a module that has seen nothing"""
    import active_gs_amd.rasterizer as R
    names = ("always_check", "skew_factor", "direct_budget_bytes", "binning_mode")
    saved = {k: R.get_option(k) for k in names}
    R.reset_state()
    yield R
    R.reset_state()
    for k, v in saved.items():
        R.set_option(k, v)


def _rel_l1(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().sum() / b.abs().sum().clamp_min(1e-30))


def _cameras(V, h, w, dev, first=0):
    from active_gs_amd.camera import camera_matrices
    from active_gs_amd.synthetic import make_camera
    cams = [make_camera(first + v, h, w) for v in range(V)]
    c2w = torch.stack([c[0] for c in cams]); K = torch.stack([c[1] for c in cams])
    cm = camera_matrices(c2w, K, 0.001, 10.0)
    return c2w.to(dev), K.to(dev), {k: v.to(dev).contiguous() for k, v in cm.items()}


# ------------------------------------------------------------------ 1. ags_facade_post_backward_batch
@pytest.mark.parametrize("h,w", [(37, 53), (120, 160)])
def test_post_backward_batch_equals_single_view_calls(agslib, h, w):
    from active_gs_amd import _lib
    from active_gs_amd._lib import ptr
    dev = torch.device("cuda:0")
    V = 5
    g = torch.Generator().manual_seed(h * w)
    depth = (1.0 + 3.0 * torch.rand(V, 1, h, w, generator=g)).to(dev)
    opacity = torch.rand(V, 1, h, w, generator=g).to(dev)
    opacity[opacity < 0.15] = 0.0                    # uncovered pixels: the mask is off there
    normal_raw = torch.randn(V, 3, h, w, generator=g).to(dev)
    g_normal = torch.randn(V, 3, h, w, generator=g).to(dev)
    g_d2n = torch.randn(V, 3, h, w, generator=g).to(dev)
    g_normal[2].zero_(); g_d2n[2].zero_()            # one view without gradients
    tanx, tany = 0.6, 0.45
    lib, s = agslib, _lib.current_stream()
    for gn, gd in ((g_normal, g_d2n), (None, g_d2n), (g_normal, None)):
        d_nr = torch.full((V, 3, h, w), float("nan"), device=dev)
        d_dep = torch.zeros(V, 1, h, w, device=dev)
        _lib.check(lib.ags_facade_post_backward_batch(V, h, w, tanx, tany, ptr(normal_raw), ptr(depth), ptr(opacity), ptr(gn),
                                                      ptr(gd), ptr(d_nr), ptr(d_dep), s), "ags_facade_post_backward_batch")
        ref_nr = torch.full((V, 3, h, w), float("nan"), device=dev)
        ref_dep = torch.zeros(V, 1, h, w, device=dev)
        for v in range(V):
            _lib.check(lib.ags_facade_post_backward(h, w, tanx, tany, ptr(normal_raw[v]), ptr(depth[v]), ptr(opacity[v]),
                                                    ptr(None if gn is None else gn[v]), ptr(None if gd is None else gd[v]),
                                                    ptr(ref_nr[v]), ptr(ref_dep[v]), s), "ags_facade_post_backward")
        torch.cuda.synchronize()
        assert torch.equal(d_nr, ref_nr)
        if gd is None:
            assert not d_dep.any() and not ref_dep.any()
        else:
            assert ref_dep.abs().sum() > 0
            assert _rel_l1(d_dep, ref_dep) <= 1e-6
            assert not d_dep[2].any()                # the view without gradients stays zero
        if gn is None:
            assert not d_nr.any()


# ------------------------------------------------------------------ 2. the node against the per-view module
def _per_view(R, ins, cm, h, w, bg, cfg, masks=None):
    from diff_gaussian_rasterization_2d import GaussianRasterizationSettings, GaussianRasterizer
    dev = ins[0].device
    outs = []
    for v in range(cm["viewmatrix"].shape[0]):
        s = GaussianRasterizationSettings(
            image_height=h, image_width=w, tanfovx=float(cm["tanfov"][0, 0]), tanfovy=float(cm["tanfov"][0, 1]), bg=bg,
            scale_modifier=1.0, viewmatrix=cm["viewmatrix"][v], projmatrix=cm["projmatrix"][v], sh_degree=0,
            campos=cm["campos"][v], prefiltered=False, render_mask=masks[v] if masks is not None else torch.tensor([], device=dev),
            weight_thres=0.03, debug=False, config=cfg)
        outs.append(GaussianRasterizer(s)(ins[0], None, ins[2], ins[3], None, ins[4], ins[5], ins[6], None))
    return outs


def _batched(R, ins, cm, h, w, bg, cfg, masks=None):
    return R.rasterize_batch(ins[0], ins[2], ins[3], ins[4], ins[5], ins[6], bg, cm["viewmatrix"], cm["projmatrix"], h, w,
                             float(cm["tanfov"][0, 0]), float(cm["tanfov"][0, 1]), render_masks=masks, config=cfg)


def test_rasterize_batch_equals_per_view_module(agslib, fresh_module):
    R = fresh_module
    dev = torch.device("cuda:0")
    n, h, w, V = 20000, 128, 160, 6
    a, _ = room_case(n, h, w, seed=4)
    _, _, cm = _cameras(V, h, w, dev)
    bg = torch.tensor([0.1, 0.2, 0.3, 0.0], device=dev)
    gm = torch.Generator().manual_seed(5)
    masks = (torch.rand(V, h, w, generator=gm) > 0.3).float().to(dev)
    for stats in (0.0, 1.0):
        cfg = torch.tensor([1.0, 1.0, 1.0, stats, 0.0], device=dev)
        for mk in (None, masks):
            ins = [t.to(dev) for t in oracle_inputs(a, requires_grad=False)]
            with torch.no_grad():
                c0 = R.counters()
                ref = _per_view(R, ins, cm, h, w, bg, cfg, mk)
                c1 = R.counters()
                out = _batched(R, ins, cm, h, w, bg, cfg, mk)
                c2 = R.counters()
            assert c2["batch_calls"] == c1["batch_calls"] + 1 and c2["forward_calls"] == c1["forward_calls"]
            assert c1["forward_calls"] == c0["forward_calls"] + V
            for v in range(V):
                for k in (0, 1, 2, 3, 4, 6, 7):
                    assert torch.equal(out[k][v], ref[v][k]), (stats, mk is None, v, k)
                # importance is a float sum over pixels taken with atomics: equal up to their order
                assert _rel_l1(out[5][v], ref[v][5]) <= 1e-5 if stats else torch.equal(out[5][v], ref[v][5]), v
            assert float(out[3].sum()) > 0

    # backward: a fixed linear functional of the five images
    cfg = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0], device=dev)
    gw = torch.Generator().manual_seed(6)
    wts = [torch.randn(V, c, h, w, generator=gw).to(dev) for c in (3, 3, 1, 1, 1)]
    leaves = []
    for _ in range(2):
        ins = [t.to(dev).requires_grad_(i in (0, 2, 4, 5, 6)) for i, t in enumerate(oracle_inputs(a, requires_grad=False))]
        ins[1] = None
        leaves.append(ins)
    ref = _per_view(R, leaves[0], cm, h, w, bg, cfg)
    sum((ref[v][k] * wts[k][v]).sum() for v in range(V) for k in range(5)).backward()
    out = _batched(R, leaves[1], cm, h, w, bg, cfg)
    sum((out[k] * wts[k]).sum() for k in range(5)).backward()
    for i in (0, 2, 4, 5, 6):
        assert leaves[0][i].grad is not None and leaves[1][i].grad is not None
        assert leaves[1][i].grad.shape == leaves[0][i].grad.shape
        assert _rel_l1(leaves[1][i].grad, leaves[0][i].grad) <= GRAD_TOL, (i, _rel_l1(leaves[1][i].grad, leaves[0][i].grad))


def test_rasterize_batch_gradients_match_the_oracle(agslib, fresh_module):
    """A small scene against the CPU oracle's autograd (per view, summed): the contract tolerances of the parity suite."""
    import _parity
    from oracle.surfel_oracle import OracleSettings, rasterize
    R = fresh_module
    dev = torch.device("cuda:0")
    n, h, w, V = 1500, 64, 80, 3
    a, _ = room_case(n, h, w, seed=8, scale_mult=2.0)
    _, _, cm = _cameras(V, h, w, dev)
    bg = torch.tensor([0.1, 0.2, 0.3, 0.0])
    cfg = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0])
    gw = torch.Generator().manual_seed(9)
    wts = [torch.randn(V, c, h, w, generator=gw) for c in (3, 3, 1, 1, 1)]
    ins = oracle_inputs(a, requires_grad=True)
    for v in range(V):
        S = OracleSettings(h, w, float(cm["tanfov"][0, 0]), float(cm["tanfov"][0, 1]), bg, 1.0, cm["viewmatrix"][v].cpu(),
                           cm["projmatrix"][v].cpu(), campos=cm["campos"][v].cpu(), config=cfg)
        o = rasterize(*ins, S)
        sum((o[k] * wts[k][v]).sum() for k in range(5)).backward()
    gin = [t.detach().clone().to(dev).requires_grad_(t.requires_grad) for t in ins]
    out = _batched(R, gin, cm, h, w, bg.to(dev), cfg.to(dev))
    sum((out[k] * wts[k].to(dev)).sum() for k in range(5)).backward()
    names = {0: "means3D", 2: "opacities", 4: "colors", 5: "scales", 6: "rotations"}
    _parity.check_grads({names[i]: ins[i].grad for i in names}, {names[i]: gin[i].grad for i in names}, regression=False,
                        what="rasterize_batch vs oracle")


# ------------------------------------------------------------------ 3. the facade takes the batch
def _attr(a, dev, scale=1.0, grad=True):
    t = lambda x: x.to(dev).clone().requires_grad_(grad)
    return (t(a["means"]), t(a["colors"][:, None, :]), t(a["opacities"]), a["confidences"].to(dev), t(a["scales"] * scale),
            t(a["rotations"]))


def _functional(outs, seed=11):
    g = torch.Generator().manual_seed(seed)
    total = 0
    for k in range(6):
        total = total + (outs[k] * torch.randn(outs[k].shape, generator=g).to(outs[k].device)).sum()
    return total


def _check_same(outs, ref, leaves, ref_leaves, tol):
    for k in range(9):
        assert torch.equal(outs[k].detach(), ref[k].detach()), k
    for k, (x, y) in enumerate(zip(leaves, ref_leaves)):
        if x.requires_grad:
            assert _rel_l1(x.grad, y.grad) <= tol, (k, _rel_l1(x.grad, y.grad))


def test_surfel_renderer_renders_grad_views_as_one_batch(agslib, fresh_module):
    R = fresh_module
    from active_gs_amd.facade import SurfelRenderer
    dev = torch.device("cuda:0")
    n, h, w, V = 20000, 120, 160, 8
    a, _ = room_case(n, h, w, seed=1)
    c2w, K, _ = _cameras(V, h, w, dev)
    bg = torch.zeros(4, device=dev)
    leaves = _attr(a, dev)
    c0 = R.counters()
    outs = SurfelRenderer(c2w, K, leaves, bg, (0.001, 10.0), (h, w), dev).render_view_all(require_grad=True)
    c1 = R.counters()
    assert c1["batch_calls"] == c0["batch_calls"] + 1          # 8 views at 120x160: one chunk
    assert c1["forward_calls"] == c0["forward_calls"]
    _functional(outs).backward()
    ref_leaves = _attr(a, dev)
    r = SurfelRenderer(c2w, K, ref_leaves, bg, (0.001, 10.0), (h, w), dev)
    r.GRAD_BATCH = False
    ref = r.render_view_all(require_grad=True)
    c2 = R.counters()
    assert c2["batch_calls"] == c1["batch_calls"] and c2["forward_calls"] == c1["forward_calls"] + V
    _functional(ref).backward()
    assert all(o.shape == x.shape for o, x in zip(outs, ref))
    _check_same(outs, ref, leaves, ref_leaves, GRAD_TOL)


def test_surfel_renderer_grad_batch_chunks_views(agslib, fresh_module, monkeypatch):
    """A batch budget that holds three views' workspaces: 8 views are three nodes, concatenated - the same tuple."""
    R = fresh_module
    from active_gs_amd import facade, raster_api as api
    from active_gs_amd.facade import SurfelRenderer
    dev = torch.device("cuda:0")
    n, h, w, V = 5000, 96, 128, 8
    a, _ = room_case(n, h, w, seed=2)
    c2w, K, _ = _cameras(V, h, w, dev)
    bg = torch.zeros(4, device=dev)
    monkeypatch.setattr(facade, "BATCH_BYTES_BUDGET", 3 * api.workspace_bytes(n, h, w, max(1 << 16, 2 * n)))
    leaves = _attr(a, dev)
    c0 = R.counters()
    outs = SurfelRenderer(c2w, K, leaves, bg, (0.001, 10.0), (h, w), dev).render_view_all(require_grad=True)
    assert R.counters()["batch_calls"] == c0["batch_calls"] + 3
    _functional(outs).backward()
    ref_leaves = _attr(a, dev)
    r = SurfelRenderer(c2w, K, ref_leaves, bg, (0.001, 10.0), (h, w), dev)
    r.GRAD_BATCH = False
    ref = r.render_view_all(require_grad=True)
    _functional(ref).backward()
    _check_same(outs, ref, leaves, ref_leaves, GRAD_TOL)


# ------------------------------------------------------------------ 4. repair under grad
def test_grad_batch_repairs_an_outgrown_workspace_inside_the_node(agslib, fresh_module):
    R = fresh_module
    from active_gs_amd.facade import SurfelRenderer
    dev = torch.device("cuda:0")
    n, h, w, V = 20000, 120, 160, 4
    a, _ = room_case(n, h, w, view=1, seed=1)
    c2w, K, _ = _cameras(V, h, w, dev)
    bg = torch.zeros(4, device=dev)
    SurfelRenderer(c2w, K, _attr(a, dev), bg, (0.001, 10.0), (h, w), dev).render_view_all(require_grad=True)   # sizes learnt
    c0 = R.counters()
    big = _attr(a, dev, scale=40.0)
    outs = SurfelRenderer(c2w, K, big, bg, (0.001, 10.0), (h, w), dev).render_view_all(require_grad=True)
    c1 = R.counters()
    assert c1["batch_calls"] == c0["batch_calls"] + 1
    assert c1["overflows"] > c0["overflows"] and c1["repaired"] > c0["repaired"]
    _functional(outs).backward()
    R.set_option("always_check", 1)
    R.reset_state()
    big2 = _attr(a, dev, scale=40.0)
    ref = [SurfelRenderer(c2w[i:i + 1], K[i:i + 1], big2, bg, (0.001, 10.0), (h, w), dev).render_view(0, require_grad=True)
           for i in range(V)]
    for i in range(V):
        for k in range(6):
            assert torch.equal(outs[k][i].detach(), ref[i][k].detach()), (i, k)
    _functional(tuple(torch.stack([r[k] for r in ref]) for k in range(6))).backward()
    for k, (x, y) in enumerate(zip(big, big2)):
        if x.requires_grad:
            assert _rel_l1(x.grad, y.grad) <= GRAD_TOL_LARGE, (k, _rel_l1(x.grad, y.grad))


# ------------------------------------------------------------------ 5. fallbacks and lifetime
def test_grad_batch_fallbacks_and_slab_lifetime(agslib, fresh_module):
    R = fresh_module
    import diff_gaussian_rasterization_2d as module
    from active_gs_amd import raster_api as api
    from active_gs_amd.facade import SurfelRenderer
    dev = torch.device("cuda:0")
    n, h, w, V = 8000, 96, 128, 4
    a, _ = room_case(n, h, w, seed=3)
    c2w, K, _ = _cameras(V, h, w, dev)
    bg = torch.zeros(4, device=dev)
    K2 = K.clone(); K2[1, 0, 0] *= 1.2; K2[1, 1, 1] *= 1.2              # one view with another field of view
    for kw in (dict(c2w=c2w, K=K2), dict(c2w=c2w[:1], K=K[:1]), dict(c2w=c2w, K=K, rasterizer_module=module)):
        c0 = R.counters()
        outs = SurfelRenderer(kw["c2w"], kw["K"], _attr(a, dev), bg, (0.001, 10.0), (h, w), dev,
                              rasterizer_module=kw.get("rasterizer_module")).render_view_all(require_grad=True)
        outs[0].sum().backward()
        c1 = R.counters()
        assert c1["batch_calls"] == c0["batch_calls"]
        assert c1["forward_calls"] == c0["forward_calls"] + kw["c2w"].shape[0]

    # the slab is leased to the node while its graph lives and back in the pool once the graph is freed
    R.reset_state()
    outs = SurfelRenderer(c2w, K, _attr(a, dev), bg, (0.001, 10.0), (h, w), dev).render_view_all(require_grad=True)
    mine = lambda: {k: v for k, v in R.state()["batch_pooled"].items() if k[1:3] == (h, w) and k[4] == V}
    assert sum(v["count"] for v in mine().values()) == 0
    outs[0].sum().backward()
    del outs
    assert sum(v["count"] for v in mine().values()) == 1
    # a growing map re-initialises or replaces the pooled slab: the pool stays bounded
    for k, grow in enumerate((1.0, 1.5, 2.2, 3.3, 5.0)):
        m = int(n * grow)
        b, _ = room_case(m, h, w, seed=20 + k)
        outs = SurfelRenderer(c2w, K, _attr(b, dev), bg, (0.001, 10.0), (h, w), dev).render_view_all(require_grad=True)
        outs[0].sum().backward()
        del outs
        pooled = mine()
        assert 1 <= sum(v["count"] for v in pooled.values()) <= 2 * len(pooled) and len(pooled) <= 2, pooled
    assert all(k[3] in (api.BIN_DIRECT, api.BIN_TILE_SORT) for k in mine())


# ------------------------------------------------------------------ 6. the training replay on the batched path
class _TorchAdam:
    """torch.optim.Adam behind the trainer's optimiser interface (step(grads))."""

    def __init__(self, params, lrs):
        self.params = list(params)
        self.opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(self.params, lrs)], eps=1e-15)

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = g.reshape(p.shape)
        self.opt.step()
        for p in self.params:
            p.grad = None


def test_map_trainer_replays_the_train_capture_on_the_batched_path(agslib, fresh_module):
    R = fresh_module
    from active_gs_amd.map_trainer import GaussianMapTrainer
    dev = torch.device("cuda:0")
    d = torch.load(os.path.join(GOLD, "train.pt"))
    cfg = d["cfg"]
    mine = dict(bound=tuple(cfg["bound"]), scale_factor=cfg["scale_factor"], optimization_steps=cfg["optimization_steps"],
                prune_interval=cfg["prune_interval"], background=tuple(cfg["background"]),
                batch_size=cfg["sampler"]["batch_size"], active_size=cfg["sampler"]["active_size"],
                use_view_distribution=cfg["use_view_distribution"],
                lrs=dict(mean=cfg["optimizer"]["mean_lr"], scale=cfg["optimizer"]["scale_lr"],
                         rotation=cfg["optimizer"]["rotation_lr"], opacity=cfg["optimizer"]["opacity_lr"],
                         harmonic=cfg["optimizer"]["harmonic_lr"]))
    raw = {k: v.to(dev) for k, v in d["raw_init"].items()}
    frames = [{k: v.to(dev) for k, v in f.items()} for f in d["frames"]]
    t = GaussianMapTrainer(raw, frames, mine, optimizer_factory=lambda p, lrs: _TorchAdam(p, lrs))
    c0 = R.counters()
    np.random.seed(7)
    t.train()
    torch.cuda.synchronize()
    assert R.counters()["batch_calls"] > c0["batch_calls"]
    for k, ref in d["raw_final"].items():
        got, init = getattr(t, k).cpu(), d["raw_init"][k]
        diff, travel = (got - ref).abs(), (ref - init).abs().mean()
        assert diff.mean() < 2e-3 * travel, (k, float(diff.mean()), float(travel))
        assert (diff > 1e-4).float().mean() < 5e-3, k
    assert torch.allclose(t.training_performance.cpu(), d["training_performance"], rtol=1e-3, atol=1e-5)
    assert len(t.last_losses) == d["steps"] and all(np.isfinite(t.last_losses))
