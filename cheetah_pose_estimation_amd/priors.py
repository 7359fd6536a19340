"""Learned priors of the monocular "data-driven" model (config 3): the Gaussian-mixture pose prior
(acinoset_misc.py:680-714, acinoset_models.py:277-300) and the linear autoregressive motion prior
(acinoset_misc.py:291-336, acinoset_models.py:173-274).  The fitted numbers are package data
(data/priors_full_pose.npz, produced by tools/fit_priors.py with the reference's own recipe); this module only
packs them into the C-ABI struct `cpe_priors`.  Other sizes of the two models -- the reference's grid search varies the number of mixture
components and the window (run_dataset.py:814-915) -- are fitted on request with the same recipe (`fit_priors`: up to 8 components, windows of 1
to 6 frames; the sweep's window 7 is refused), from the pose table the reference ships beside its models, and cached as plain arrays."""
import os

import numpy as np

from . import abi

_NPZ = os.path.join(os.path.dirname(__file__), "data", "priors_full_pose.npz")


def load_priors(pose: bool = True, motion: bool = True, path: str = _NPZ) -> abi.Priors:
    z = np.load(path)
    pr = abi.Priors()
    if pose:
        w, mu, cov = z["gmm_weights"], z["gmm_means"], z["gmm_covariances"]
        K, D = mu.shape
        assert K <= abi.MAX_GMM and D <= abi.NX
        pr.gmm_k, pr.gmm_dim = K, D
        for k in range(K):
            sign, logdet = np.linalg.slogdet(cov[k])
            assert sign > 0
            pr.gmm_logw[k] = np.log(w[k]) - 0.5 * (D * np.log(2 * np.pi) + logdet)     # log of w_k / sqrt(det(2 pi Sigma_k))
            P = np.linalg.inv(cov[k])
            P = 0.5 * (P + P.T)
            for i in range(D):
                pr.gmm_mu[k][i] = mu[k, i]
                for j in range(D):
                    pr.gmm_P[k][i][j] = P[i, j]
    if motion:
        coef, b, var = z["lr_coef"], z["lr_intercept"], z["lr_error_variance"]
        W = int(z["lr_window"])
        assert W <= abi.MAX_WINDOW and coef.shape == (abi.NX, W * abi.NX)
        pr.lr_window = W
        for p in range(abi.NX):
            pr.lr_b[p] = b[p]
            pr.lr_w[p] = 0.0 if var[p] == 0 else 1.0 / var[p]                           # acinoset_misc.py:307
            for j in range(W * abi.NX):
                pr.lr_coef[p][j] = coef[p, j]
    return pr


def _supervised_xy(data: np.ndarray, starts: np.ndarray, window: int):
    """the reference's framing (MotionModel._read_dataset, acinoset_models.py:246-274): per recorded run, rows [x_{t-window} ... x_{t-1} | x_t]"""
    def frame(seg):
        n = seg.shape[0]
        if n <= window:
            return np.zeros((0, seg.shape[1] * (window + 1)))
        return np.concatenate([seg[i:n - window + i] for i in range(window + 1)], axis=1)
    parts, end = [], 0
    for b, e in zip(starts, starts[1:]):
        parts.append(frame(data[b:e])); end = e
    parts.append(frame(data[end:]))
    xy = np.concatenate(parts)
    nv = data.shape[1]
    return xy[:, :nv * window], xy[:, nv * window:]


def fit_priors(n_components: int = 5, window: int = 4, sparse: bool = True, dataset: str = None, cache_dir: str = None) -> str:
    """Fit the two learned models at another size, exactly as the reference does at run time -- GaussianMixture(n_components, random_state=42,
    max_iter=20000) on the 22 relative angles (acinoset_models.py:277-300) and MultiTaskLasso(alpha=1e-2, random_state=42, max_iter=20000) or, with
    sparse=False, LinearRegression() on the window framing of the 28 pose variables, weights 1 / var(training residual) (acinoset_models.py:173-225) --
    on `dataset` (default ./models/data-driven/dataset_full_pose.csv: the reference reads the .h5 beside it relative to its working directory,
    acinoset_misc.py:298, :685; the .csv twin holds the same table and needs no PyTables).  Returns the path of an .npz of plain arrays in the layout
    of the packaged file (for load_priors(path=...)); fitted once per size and cached.  Needs scikit-learn and pandas, like the reference."""
    if not (1 <= n_components <= abi.MAX_GMM):
        raise NotImplementedError(f"pose prior with {n_components} components: cpe_priors holds at most {abi.MAX_GMM}")
    if not (1 <= window <= abi.MAX_WINDOW):
        raise NotImplementedError(f"motion prior with a window of {window} frames: cpe_priors and the solver's band hold windows of 1 to {abi.MAX_WINDOW} frames")
    cache_dir = cache_dir or os.environ.get("CPE_CACHE_DIR") or os.path.join(os.path.expanduser("~"), ".cache", "cheetah_pose_estimation_amd")
    out = os.path.join(cache_dir, f"priors_k{n_components}_w{window}_{'lasso' if sparse else 'dense'}.npz")
    if os.path.isfile(out):
        return out
    dataset = dataset or os.path.join(".", "models", "data-driven", "dataset_full_pose.csv")
    if not os.path.isfile(dataset):
        raise FileNotFoundError(f"{dataset}: the pose table of the reference (models/data-driven/dataset_full_pose.csv) is needed to fit priors of another size")
    import pandas as pd
    from sklearn.linear_model import LinearRegression, MultiTaskLasso
    from sklearn.mixture import GaussianMixture
    df = pd.read_csv(dataset, index_col=0)
    data = df.iloc[:, :abi.NX].to_numpy()
    X, y = _supervised_xy(data, np.where(df.index.values == 0)[0], window)
    lr = (MultiTaskLasso(alpha=1e-2, random_state=42, max_iter=20000) if sparse else LinearRegression()).fit(X, y)
    err_var = np.var(y - lr.predict(X), axis=0)
    gmm = GaussianMixture(n_components=n_components, random_state=42, max_iter=20000).fit(data[:, 6:abi.NX])
    os.makedirs(cache_dir, exist_ok=True)
    tmp = out + f".{os.getpid()}.tmp.npz"
    np.savez_compressed(tmp, lr_coef=lr.coef_, lr_intercept=lr.intercept_, lr_error_variance=err_var, lr_window=window,
                        gmm_weights=gmm.weights_, gmm_means=gmm.means_, gmm_covariances=gmm.covariances_)
    os.replace(tmp, out)
    return out
