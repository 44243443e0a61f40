"""-m gpu: every link of the U-Net++ and classifier graphs (tests/graph_links.py: references, allowances and their sources) on the engine's own stored tensors.

One forward + backward per case; every materialised activation, every gradient tap and every parameter gradient is then compared, element by element, with the
float64 function of the engine's own stored inputs -- so a wrong buffer, slice, stride, seed, count or mask mode in build_programs_pp / build_programs_cls fails
exactly the link it sits in, where the engine-against-engine comparisons of test_gpu_bf16_model.py see a cosine above 0.9.  tests/test_graph_links_host.py shows on
the CPU that ten kinds of planted wiring error each fail a named link.  Every case asserts that each op name of both programs belongs to a link that ran and that
every key of get_grads() was checked: a future fused op with no link fails there.

Cases: U-Net++ bf16 at (2, 32, 32) and (3, 24, 40) (the shapes of the fp32 test: two / three images, a ragged width, four levels), dropout off and on (any rate > 0
switches the graph's fixed 0.2 / 0.4 rates on); classifier bf16 at (4, 32, 32) and (5, 24, 40) with class weights (0.8, 1.4), dropout 0 and 0.4, and once with
options={"bn_fold": 3}; both link tables once in fp32 at the smallest shape, against the engine the oracle tests already hold.  `bound-ratio link ...` lines: -s.

Measured on an MI355X (worst error / allowance over the eleven cases; no link fails, so the tests found no wiring defect in either builder):
  bf16 tensors: the midpoint allowance is used by 4e-4 of the 21.7 M compared elements; largest |ref - midpoint| / tol among them 0.089 (head backward into
  x1_4), 0.052 (data gradient x1_4a > cat_x1_4), 0.051 (first conv).  A gradient buffer written by several launches prints 1 by construction: its reference is the
  centre of the interval [lo, hi] of graph_links.grad_sum, and an element that sits on an end of it is at the edge of the allowance.
  fp32 outputs: loss / f1 0.68 (one fp32 rounding of the quotient), fc1/kernel 0.52, conv kernels <= 0.43 (c4b/kernel), head into h1 0.26, everything else
  below 0.25; on the fp32 engine the accumulated buffers 0.48 (c1), 0.33 (x1_2), the data gradient c1b > bn1a 0.33.
Wall time: 4.9 s for the eleven cases."""
import numpy as np
import pytest

import graph_links as G

pytestmark = pytest.mark.gpu


def run_case(arch, n, h, w, dtype, dropout, options=None, seed=7):
    from covidseg_amd.engine import HipUNet
    rng = np.random.default_rng(100 * n + h + w)
    wts = G.case_weights(arch, seed, (h, w))
    x = rng.random((n, h, w, 1)).astype(np.float32)
    cw = (1.0, 1.0)
    eng = HipUNet(h, w, 1, arch=arch, dropout_rate=dropout, seed=seed, dtype=dtype, options=options)
    if arch == "classifier":
        y = (rng.random(n) > 0.5).astype(np.float32); y[0], y[1] = 0.0, 1.0
        cw = (0.8, 1.4)
        eng.set_class_weights(*cw)
    else:
        y = (np.round(rng.random((n, h, w, 1)) ** 4 * 255) / 255).astype(np.float32)
    eng.set_weights(wts)
    src = G.engine_src(eng, x, y, wts, cw)
    L = G.Links(src, collect=True).run()          # (all links run, so that one report names every link that fails)
    assert not L.failed, f"{len(L.failed)} of {len(L.ran)} links fail: " + " || ".join(f"{k}: {v[:300]}" for k, v in L.failed.items())
    L.assert_complete()
    return src, L


@pytest.mark.parametrize("dropout", [0.0, 0.3])
@pytest.mark.parametrize("shape", [(2, 32, 32), (3, 24, 40)])
def test_unetpp_bf16_links(shape, dropout):
    src, L = run_case("unetpp", *shape, "bf16", dropout)
    assert src.folded == {n[0] + "b" for n in G.O.PP_NODES}                      # the default graph: every conv_block's first BatchNorm is folded
    assert any(k.startswith("bwd sum >c1: pool | skip:x1_4+skip:x1_3+skip:x1_2") for k in L.ran), sorted(L.ran)


@pytest.mark.parametrize("dropout", [0.0, 0.4])
@pytest.mark.parametrize("shape", [(4, 32, 32), (5, 24, 40)])
def test_classifier_bf16_links(shape, dropout):
    src, L = run_case("classifier", *shape, "bf16", dropout)
    assert src.fused_tail


def test_classifier_bf16_links_with_the_16_channel_block_folded():
    src, L = run_case("classifier", 4, 32, 32, "bf16", 0.0, options={"bn_fold": 3})
    assert "c1b" in src.folded


@pytest.mark.parametrize("arch,shape", [("unetpp", (2, 32, 32)), ("classifier", (4, 32, 32))])
def test_the_link_tables_hold_on_the_fp32_engine(arch, shape):
    run_case(arch, *shape, "fp32", 0.0)
