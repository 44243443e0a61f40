"""The routed two-model system the reference works towards (the comment above T1:1386): slices are clustered by their bottleneck features, one
U-Net is trained per cluster, and a new slice is first assigned to a cluster whose model then predicts its mask.

ClusterRoutedModel(base) wraps a trained UNetModel (U-Net or U-Net++):
  fit_router(x)   feature_matrix -> PCA -> KMeans on x, as the runner's cluster step does (T1:1386-1424), then a cluster.Router
  fit(x, y)       route x, then train one expert UNetModel per cluster on its rows (starting from the base weights or a fresh seed)
  predict(x)      per batch: the base forward, unet_cluster_route on its tap (projection + nearest centre), one predict_batch per non-empty group
                  of its expert, the results scattered back into input order
  evaluate(x, y)  the routed whole-set scores and each expert's own evaluate on its routed rows
  save / load     base.h5, expert_{j}.h5 (the Keras HDF5 writer), router.npz and manifest.json in one directory
"""
from __future__ import annotations

import json
import os

import numpy as np

from . import weights as W
from .keras_like import UNetModel, binary_matches, dp_info, load_model, sm_scores, _host

MANIFEST_FORMAT = 1


def _engine_layer(model, layer):
    rev = {v.split("/")[0]: k.split("/")[0] for k, v in W.keras_names(model.in_ch, model.arch).items()}
    return rev.get(layer, layer)


def _router_device():
    import torch
    return "cuda" if torch.cuda.is_available() else "cpu"


def _prefixed(path, j):
    """the checkpoint path of expert j: `cluster{j}_` in front of the file name"""
    d, f = os.path.split(path)
    return os.path.join(d, f"cluster{j}_{f}")


class ClusterRoutedModel:
    """base: a trained UNetModel; layer: the tap (Keras or engine name); n_components / n_clusters / random_state: PCA(n_components) and
    KMeans(n_clusters, random_state) as in T1:1415-1422.  Single process only (a data-parallel base is a ValueError)."""

    def __init__(self, base, layer="conv2d_9", n_components=1000, n_clusters=2, random_state=0):
        if getattr(base, "arch", None) not in ("unet", "unetpp"):
            raise ValueError(f"ClusterRoutedModel: the base must be a U-Net or U-Net++ UNetModel, not arch {getattr(base, 'arch', None)!r}")
        if dp_info(base.backend)[0] > 1:
            raise ValueError("ClusterRoutedModel: data-parallel backends (world size > 1) are not supported; route on a single-process model")
        self.base = base
        self.layer = layer
        self.n_components, self.n_clusters, self.random_state = int(n_components), int(n_clusters), random_state
        self.router = None
        self.experts = [base] * self.n_clusters
        self.expert_source = ["base"] * self.n_clusters
        self._tap_name = _engine_layer(base, layer)

    # --- the router ------------------------------------------------------------------------------------------------------------------------
    def fit_router(self, x, batch_size=32):
        """T1:1386-1422: features of every slice of x, PCA(min(n_components, n - 1, d)), KMeans(n_clusters, random_state); then the Router."""
        from .cluster import PCA, KMeans
        data = self.base.feature_matrix(self.layer, x, batch_size=batch_size)
        k = min(self.n_components, data.shape[0] - 1, data.shape[1])
        pca = PCA(n_components=k).fit(data)
        kmeans = KMeans(n_clusters=self.n_clusters, random_state=self.random_state).fit(pca.transform(data))
        hwc = self.base.intermediate_output(self.layer, x[:1]).shape[1:]
        return self.set_router(pca, kmeans, hwc)

    def set_router(self, pca, kmeans, tap_shape, device=None):
        """Build the Router from an already fitted PCA and KMeans (the runner's cluster step)."""
        from .cluster import Router
        self.router = Router(pca, kmeans, tap_shape, self.layer, device=device or _router_device())
        self.n_components = self.router.n_components
        return self

    def _labels_of_last(self, n):
        """Labels (int32 host array) of the last base forward of n rows.  A backend may bring its own routing (route_taps: the CPU test backends);
        the engine's is unet_cluster_route on the tap_device view."""
        be = self.base.backend
        if hasattr(be, "route_taps"):
            return np.asarray(be.route_taps(self.router, n, self._tap_name), np.int32)
        labels, _, _ = self.router.assign(be.tap_device(n, self._tap_name))
        return labels.cpu().numpy()

    def _check_router(self):
        if self.router is None:
            raise RuntimeError("ClusterRoutedModel: no router (fit_router or set_router first)")

    def route(self, x, batch_size=32):
        """The cluster of every row of x (int32)."""
        self._check_router()
        out = []
        for i in range(0, len(x), batch_size):
            xb = x[i:i + batch_size]
            self.base.backend.predict_batch(xb)
            out.append(self._labels_of_last(len(xb)))
        return np.concatenate(out) if out else np.zeros(0, np.int32)

    # --- experts ---------------------------------------------------------------------------------------------------------------------------
    def _new_expert(self, j, init):
        seed = (self.base.seed if self.base.seed is not None else 0) + 1 + j
        if not hasattr(self.base.backend, "spawn"):
            raise ValueError(f"ClusterRoutedModel: backend {type(self.base.backend).__name__} cannot build experts (it has no spawn)")
        e = UNetModel(self.base.h, self.base.in_ch, backend=self.base.backend.spawn(seed), seed=seed, arch=self.base.arch)
        e.verbose = self.base.verbose
        if init == "base":
            e.set_weights(self.base.get_weights())
        e.compile(lr=self.base.backend.lr, loss=self.base.loss, loss_kwargs=self.base.loss_config)
        return e

    def fit(self, x, y, init="base", **fit_kw):
        """Route x and train one expert per cluster on its rows with UNetModel.fit(**fit_kw); validation_data is split by the same routing and the
        checkpoint paths get a `cluster{j}_` prefix.  init: "base" (start from the base weights) or "fresh" (a fresh seed).  Every expert has the base
        model's size, graph, dtype, options and compiled loss.  expert_source[j]: "trained-from-base" / "trained-from-fresh", or "base" for a
        cluster without training rows, which keeps the base model as its expert.
        Returns the per-cluster History (None for such a cluster)."""
        if init not in ("base", "fresh"):
            raise ValueError(f"fit(init={init!r}): 'base' or 'fresh'")
        self._check_router()
        labels = self.route(x)
        vd = fit_kw.pop("validation_data", None)
        vlab = self.route(vd[0]) if vd is not None else None
        hists = []
        for j in range(self.n_clusters):
            sel = np.where(labels == j)[0]
            if len(sel) == 0:
                print(f"cluster {j} has no training rows: the base model is its expert")
                self.experts[j], self.expert_source[j] = self.base, "base"
                hists.append(None)
                continue
            e = self._new_expert(j, init)
            kw = dict(fit_kw)
            for key in ("checkpoint_dice", "checkpoint_loss"):
                if kw.get(key):
                    kw[key] = _prefixed(kw[key], j)
            if vd is not None:
                vs = np.where(vlab == j)[0]
                kw["validation_data"] = (vd[0][vs], vd[1][vs]) if len(vs) else None
            hists.append(e.fit(x[sel], y[sel], **kw))
            self.experts[j], self.expert_source[j] = e, f"trained-from-{init}"
        return hists

    # --- inference -------------------------------------------------------------------------------------------------------------------------
    def _routed_batches(self, x, batch_size):
        """(start, routed probabilities of the batch (as the backend returns them), labels) for every batch of x"""
        self._check_router()
        for i in range(0, len(x), batch_size):
            xb = x[i:i + batch_size]
            p_base, _ = self.base.backend.predict_batch(xb)
            lab = self._labels_of_last(len(xb))
            if hasattr(p_base, "detach"):
                import torch
                out = torch.empty_like(p_base)
            else:
                out = np.empty_like(np.asarray(p_base))
            for j in range(self.n_clusters):
                idx = np.where(lab == j)[0]
                if len(idx) == 0:
                    continue
                xg = xb[idx] if len(idx) < len(xb) else xb
                p, _ = self.experts[j].backend.predict_batch(xg)
                if hasattr(out, "index_copy_"):
                    out.index_copy_(0, torch.from_numpy(idx).to(out.device), p.to(out.dtype))
                else:
                    out[idx] = np.asarray(p)
            yield i, out, lab

    def predict(self, x, batch_size=32):
        """Routed model.predict: the same shape and order as UNetModel.predict."""
        outs = [(o.detach().cpu().numpy() if hasattr(o, "detach") else np.asarray(o)) for _, o, _ in self._routed_batches(x, batch_size)]
        return np.concatenate(outs, 0)

    def evaluate(self, x, y, batch_size=32, thresholds=(0.547,), accuracy=True):
        """{"whole": dice / iou / precision / recall per threshold on the routed probabilities (threshold_sums per batch, averaged over batches
        as UNetModel.evaluate does) and, with accuracy, Keras' binary accuracy over every pixel of the set; "per_cluster": for cluster j,
        [loss, FScore@thresholds[0], IOUScore@thresholds[0]] (+ [accuracy]) from expert j's own evaluate on the rows routed to j (None when
        no row is), "labels": the routing, "counts"}.  There is no whole-set loss: the experts' loss heads cannot be mixed inside one batch."""
        thresholds = list(thresholds)
        be = self.base.backend
        per_batch, matches, pixels, labels = [], [], 0, []
        for i, p, lab in self._routed_batches(x, batch_size):
            yb = y[i:i + batch_size]
            labels.append(lab)
            if thresholds:
                per_batch.append(be.threshold_sums(p, yb, thresholds))
            if accuracy:
                matches.append(binary_matches(p, yb)); pixels += int(np.prod(p.shape))
        whole = {}
        if per_batch:
            sc = [sm_scores(s[:, 0], s[:, 1], s[:, 2]) for s in (_host(b) for b in per_batch)]
            for k in ("dice", "iou", "precision", "recall"):
                whole[k] = np.mean([b[k] for b in sc], axis=0)
        if accuracy:
            whole["accuracy"] = sum(int(m) for m in matches) / pixels if pixels else float("nan")
        labels = np.concatenate(labels) if labels else np.zeros(0, np.int32)
        per = []
        for j in range(self.n_clusters):
            sel = np.where(labels == j)[0]
            if len(sel) == 0:
                per.append(None)
                continue
            ev = self.experts[j].evaluate(x[sel], y[sel], batch_size=batch_size, thresholds=thresholds[:1] or None, accuracy=accuracy)
            row = [float(ev["loss"])]
            if thresholds:
                row += [float(ev["dice"][0]), float(ev["iou"][0])]
            if accuracy:
                row.append(float(ev["accuracy"]))
            per.append(row)
        return {"whole": whole, "per_cluster": per, "labels": labels, "counts": np.bincount(labels, minlength=self.n_clusters).tolist()}

    # --- persistence -----------------------------------------------------------------------------------------------------------------------
    def save(self, directory):
        """directory/base.h5, expert_{j}.h5 (UNetModel.save), router.npz (components and mean in the reference's (C, H, W) order, centres, tap
        shape, layer, explained variance ratio, format) and manifest.json."""
        self._check_router()
        os.makedirs(directory, exist_ok=True)
        self.base.save(os.path.join(directory, "base.h5"))
        for j, e in enumerate(self.experts):
            if e is not self.base:
                e.save(os.path.join(directory, f"expert_{j}.h5"))
        np.savez(os.path.join(directory, "router.npz"), **self.router.arrays())
        be = self.base.backend
        man = {"format": MANIFEST_FORMAT, "layer": self.layer, "n_components": self.n_components, "n_clusters": self.n_clusters,
               "random_state": self.random_state, "expert_source": list(self.expert_source), "arch": self.base.arch, "input_size": self.base.h,
               "in_ch": self.base.in_ch, "engine": {"dtype": getattr(be, "dtype", None) if isinstance(getattr(be, "dtype", None), str) else None,
                                                    "options": getattr(be, "options", None)}}
        with open(os.path.join(directory, "manifest.json"), "w") as f:
            json.dump(man, f, indent=1)

    @classmethod
    def load(cls, directory, backend=None, **backend_kw):
        """The model save() wrote.  backend: None (engines built from the manifest's dtype / options, plus backend_kw) or a callable returning a
        fresh backend for each of the base and the experts."""
        with open(os.path.join(directory, "manifest.json")) as f:
            man = json.load(f)
        if man.get("format") != MANIFEST_FORMAT:
            raise ValueError(f"{directory}: manifest format {man.get('format')!r}, this version reads {MANIFEST_FORMAT}")
        z = np.load(os.path.join(directory, "router.npz"))
        if int(z["format"]) != 1:
            raise ValueError(f"{directory}: router.npz format {int(z['format'])}, this version reads 1")
        kw = dict(backend_kw)
        if backend is None:
            eng = man.get("engine") or {}
            if eng.get("dtype") and "dtype" not in kw:
                kw["dtype"] = eng["dtype"]
            if eng.get("options") and "options" not in kw:
                kw["options"] = eng["options"]

        def one(name):
            return load_model(os.path.join(directory, name), backend=backend() if backend is not None else None, **kw)
        base = one("base.h5")
        m = cls(base, layer=man["layer"], n_components=man["n_components"], n_clusters=man["n_clusters"], random_state=man["random_state"])
        m.expert_source = list(man["expert_source"])
        for j, src in enumerate(m.expert_source):
            m.experts[j] = base if src == "base" else one(f"expert_{j}.h5")
        from .cluster import Router
        evr = z["explained_variance_ratio"]
        m.router = Router.from_arrays(z["components"], z["mean"], z["centres"], tuple(int(v) for v in z["tap_shape"]), str(z["layer"]),
                                      evr if evr.size else None, device=_router_device())
        return m
