"""CP multinomial logistic tensor regression on MI355X — drop-in for the reference's
`multinomial_tensor_regression.py` (kimerein/tensor_regression).

Same helpers, `model`, `CP_logistic_regression` class and semantics — including the
reference's double softmax (the model returns probabilities and CrossEntropyLoss applies
log-softmax to them again, multinomial_tensor_regression.py:180-187 + :448-450) — with the
hot path (factor prep, X·B over all classes, softmax, weighted CE, X^T·dZ, MTTKRP, Adam)
running as gfx950 HIP kernels through the C ABI.
"""
import types

import numpy as np
import torch

from . import _engine, _fit, _lib, _many
from ._engine import Plan, as_device_f32, adam_hparams, run_adam_fit
from .standard_tensor_regression import _plan_for, L2_penalty  # noqa: F401  (L2_penalty re-exported)

__all__ = ["squeeze_integers", "confusion_matrix", "idx_to_oneHot", "make_BcpInit", "non_neg_fn", "model",
           "L2_penalty", "CP_logistic_regression", "predict_many", "score_many", "fit_Adam_many"]


####################################
######## Useful functions ##########
####################################

def squeeze_integers(intVec):
    """Relabel integers to consecutive ids from 0 (multinomial…py:18-37)."""
    intVec = np.asarray(intVec)
    uniques = np.unique(intVec)
    return np.searchsorted(uniques, intVec)


def confusion_matrix(y_hat, y_true):
    """Column-normalised confusion matrix (multinomial…py:45-65)."""
    n_classes = np.max(y_true) + 1
    if y_hat.ndim == 1:
        y_hat = idx_to_oneHot(y_hat, n_classes)
    cmat = y_hat.T @ idx_to_oneHot(y_true, n_classes)
    return cmat / np.sum(cmat, axis=0)[None, :]


def idx_to_oneHot(arr, n_classes=None):
    """(multinomial…py:67-86)"""
    if n_classes is None:
        n_classes = np.max(arr) + 1
    oneHot = np.zeros((arr.size, n_classes))
    oneHot[np.arange(arr.size), arr] = 1
    return oneHot


def make_BcpInit(B_dims, rank, non_negative, scale=1, device='cpu'):
    """Uniform init rand*scale - (1-nn)*scale/2, requires_grad (multinomial…py:88-114)."""
    Bcp_init = [(torch.rand((B_dims[ii], rank)) * scale - (1 - non_negative[ii]) * (scale / 2)).to(device)
                for ii in range(len(B_dims))]
    for ii in range(len(B_dims)):
        Bcp_init[ii].requires_grad = True
    return Bcp_init


def non_neg_fn(B_cp, non_negative, softplus_kwargs=None):
    """(multinomial…py:116-146)"""
    if softplus_kwargs is None:
        softplus_kwargs = {'beta': 50, 'threshold': 1}
    for ii in range(len(B_cp)):
        if non_negative[ii]:
            yield torch.nn.functional.softplus(B_cp[ii], **softplus_kwargs)
        else:
            yield B_cp[ii]


def model(X, Bcp, weights, non_negative, softplus_kwargs=None):
    """softmax(inner(X, cp_to_tensor((weights, non_neg_fn(Bcp))), n_modes=len(Bcp)-1), dim=1)
    (multinomial_tensor_regression.py:148-187) on the gfx950 forward kernel; returns (N, C)."""
    if not isinstance(X, torch.Tensor) or X.device.type != "cuda":
        raise ValueError("model: X must be a torch tensor on a HIP device (device='cuda')")
    K = len(Bcp) - 1
    if X.ndim != K + 1 or list(X.shape[1:]) != [int(A.shape[0]) for A in Bcp[:-1]]:
        raise ValueError(f"Incorrect shapes for inner product along {K} common modes. "
                         f"tensor_1.shape={list(X.shape)}, factors={[tuple(A.shape) for A in Bcp]}")
    dev = X.device
    C, rank = int(Bcp[-1].shape[0]), int(Bcp[0].shape[1])
    plan = _plan_for(_lib.TR_MODEL_MULTINOMIAL, X.shape[1:], C, rank, 1, non_negative, softplus_kwargs, dev)
    arena = plan.pack([torch.as_tensor(A).to(dev) for A in Bcp])
    w = torch.as_tensor(weights, dtype=torch.float32).to(dev).contiguous()
    return plan.forward(_engine.as_device_rows(X, dev.index), arena, w)


####################################
########### Main class #############
####################################

class CP_logistic_regression():
    _takes_host_stream = True  # (the hierarchical module's constructor does not)

    def __init__(self, X, y, rank=5, non_negative=False, weights=None, Bcp_init=None, Bcp_init_scale=1,
                 device='cpu', softplus_kwargs=None):
        """(multinomial_tensor_regression.py:212-286; same arguments and attributes).  X may also
        be a util.HostStream (host-resident X streamed through HBM every iteration; fit_Adam and
        predict only)."""
        from .util import HostStream
        self.X = X if self._takes_host_stream and isinstance(X, HostStream) else \
            torch.as_tensor(X, dtype=torch.float32).to(device)
        self.y = torch.as_tensor(y, dtype=torch.long).to(device)
        if weights is None:
            self.weights = torch.ones((rank), device=device)
        else:
            self.weights = torch.tensor(weights)
        self.softplus_kwargs = _fit.softplus_or_default(softplus_kwargs)
        self.rank = rank
        self.device = device
        self.non_negative = _fit.non_negative_flags(non_negative, self.X.ndim)
        self.n_classes = len(torch.unique(self.y))
        B_dims = np.concatenate((np.array(self.X.shape[1:]), [self.n_classes]))
        # a class factor drawn here from the LOCAL labels may be widened to the global class set
        # by a sharded fit_Adam (_sync_class_set); one passed in by the caller is never resized
        self._class_factor_auto = Bcp_init is None
        self._Bcp_init_scale = Bcp_init_scale
        if Bcp_init is None:
            self.Bcp = make_BcpInit(B_dims, self.rank, self.non_negative, scale=Bcp_init_scale, device=self.device)
        else:
            self.Bcp = Bcp_init
        self.loss_running = []
        self._plan = None
        self._dev_cache = None

    def return_self(self):
        return self.Bcp

    # ---- plumbing ------------------------------------------------------------------------------
    def _device_data(self):
        from .util import HostStream
        hs = isinstance(self.X, HostStream)
        dev = self.X.dev_index if hs else _engine.compute_device(self.X, self.device)
        c = self._dev_cache
        if c is None or c[0] != dev or c[1] is not self.X or c[2] is not self.y:
            Xd = self.X if hs else _engine.as_device_rows(self.X, dev)
            yd = self.y.to(f"cuda:{dev}", torch.long).contiguous()
            C = int(self.Bcp[-1].shape[0])
            ymin, ymax = int(yd.min().item()), int(yd.max().item())
            if ymin < 0 or ymax >= C:
                raise IndexError(f"Target {ymax if ymax >= C else ymin} is out of bounds.")
            self._dev_cache = (dev, self.X, self.y, Xd, yd)
        return self._dev_cache[0], self._dev_cache[3], self._dev_cache[4]

    def _get_plan(self, Xd, rows):
        from .util import HostStream
        if isinstance(Xd, HostStream):
            rows = min(rows, Xd.chunk_rows)
        dims = [int(A.shape[0]) for A in self.Bcp[:-1]]
        if list(Xd.shape[1:]) != dims:
            raise ValueError(f"Incorrect shapes for inner product along {len(dims)} common modes. "
                             f"tensor_1.shape={list(Xd.shape)}, factors={[tuple(A.shape) for A in self.Bcp]}")
        C, R = int(self.Bcp[-1].shape[0]), int(self.Bcp[0].shape[1])
        p = self._plan
        if (p is None or p.max_rows < rows or p.feature_dims != dims or p.n_classes != C or p.rank != R
                or p.dev != _engine.device_index(Xd.device)
                or p.nonlin != _engine.nonlin_key(self.non_negative, self.softplus_kwargs, len(dims) + 1)):
            p = Plan(_lib.TR_MODEL_MULTINOMIAL, dims, C, R, rows, self.non_negative, self.softplus_kwargs,
                     Xd.device)
            self._plan = p
        return p

    def _sync_class_set(self, process_group):
        """The class set of a sample-sharded fit is the union of every rank's labels.

        The reference takes n_classes = len(unique(y)) from the data it is given
        (multinomial_tensor_regression.py:279-280) and CrossEntropyLoss then requires every label
        to be < n_classes.  A rank's shard may miss classes, so under a process group the count is
        taken from all ranks' labels (MAX all-reduce of the label range, then of a presence
        bitmap), and every rank raises the reference's own error when the union is not
        0..C-1 — the same error a single process on the concatenated data would raise.  A class
        factor this model drew from its local labels is widened to the global count (the new rows
        drawn like make_BcpInit's); the fit then starts every rank from group rank 0's parameters
        (sync_replicas).  A caller's Bcp_init keeps its shape, and must cover the labels."""
        import torch.distributed as dist
        cdev = _engine.collective_device(process_group)
        y = torch.as_tensor(self.y).reshape(-1).to(cdev, torch.long)
        n = y.numel()
        # label range and every rank's sample count in one MAX all-reduce (the counts in per-rank
        # slots, -1 elsewhere)
        world, me = dist.get_world_size(process_group), dist.get_rank(process_group)
        rng = torch.full((2 + world,), -1, dtype=torch.int64)
        rng[0], rng[1], rng[2 + me] = (int(y.max()) if n else -1), (-int(y.min()) if n else 0), n
        rng = rng.to(cdev)
        dist.all_reduce(rng, op=dist.ReduceOp.MAX, group=process_group)
        r = rng.tolist()
        ymax, ymin, n_all = r[0], -r[1], sum(r[2:])
        if n_all == 0:
            raise ValueError("the sharded multinomial fit got no samples on any rank")
        if ymin < 0:
            raise IndexError(f"Target {ymin} is out of bounds.")
        if ymax >= n_all:  # fewer samples than label values: the union cannot be 0..ymax
            raise IndexError(f"Target {ymax} is out of bounds.")
        present = torch.zeros(ymax + 1, dtype=torch.int32, device=cdev)
        if n:
            present[y] = 1
        dist.all_reduce(present, op=dist.ReduceOp.MAX, group=process_group)
        C = int(present.sum())
        if self._class_factor_auto:
            if C != ymax + 1:  # reference: n_classes = C < ymax + 1 -> label ymax out of bounds
                raise IndexError(f"Target {ymax} is out of bounds.")
            A = self.Bcp[-1]
            if int(A.shape[0]) != C:
                extra = (torch.rand((C - int(A.shape[0]), self.rank)) * self._Bcp_init_scale
                         - (1 - self.non_negative[-1]) * (self._Bcp_init_scale / 2)).to(A.device)
                with torch.no_grad():
                    self.Bcp[-1] = torch.cat([A.detach(), extra.to(A.dtype)], dim=0).requires_grad_(True)
                self._plan = None
                self._dev_cache = None
                self._cw_cache = None
            self.n_classes = C
        Cm = int(self.Bcp[-1].shape[0])
        _engine.check_uniform(Cm, process_group, "the number of classes (class-factor rows)", cdev)
        if ymax >= Cm:
            raise IndexError(f"Target {ymax} is out of bounds.")

    def _class_weights(self, weights, dev, yd):
        """The class weights on the device and this rank's CE normaliser sum_n w[y_n].  Both are
        kept for the next fit on the same labels and weights (the normaliser costs a reduction
        over the labels and a host synchronisation)."""
        cwh = torch.as_tensor(weights, dtype=torch.float32).detach().cpu()
        C = int(self.Bcp[-1].shape[0])
        if cwh.ndim != 1 or cwh.numel() != C:
            raise RuntimeError(f"weight tensor should be defined either for all {C} classes or no classes "
                               f"but got weight tensor of shape: {list(cwh.shape)}")
        key = (yd, yd._version, dev, cwh.numpy().tobytes())
        c = getattr(self, "_cw_cache", None)
        if c is not None and c[0] is key[0] and c[1:4] == key[1:]:
            return c[4], c[5]
        cw = cwh.to(f"cuda:{dev}").contiguous()
        W = float(cw.double()[yd].sum().item())
        self._cw_cache = key + (cw, W)
        return cw, W

    # ---- fitting -------------------------------------------------------------------------------
    def fit(self, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, weights=None, verbose=False,
            running_loss_logging_interval=10, LBFGS_kwargs=None):
        """LBFGS fit (multinomial_tensor_regression.py:291-387); closures evaluated on gfx950."""
        _fit.require_lbfgs_kwargs(LBFGS_kwargs)
        dev, Xd, yd = self._device_data()
        if not isinstance(Xd, torch.Tensor):
            raise NotImplementedError("the LBFGS fit needs X resident on the device (use fit_Adam for a HostStream)")
        plan = self._get_plan(Xd, Xd.shape[0])
        cw, W = self._class_weights(weights, dev, yd)
        w = self.weights.to(f"cuda:{dev}", torch.float32).contiguous()
        grad, gtot, loss_out = _fit.lbfgs_buffers(plan, dev)

        def closure_loss():
            arena = plan.pack(self.Bcp)
            plan.loss_grad(Xd, yd, cw, W, arena, w, grad)
            plan.finalize_grad(arena, grad, lambda_L2, gtot, loss_out)
            _fit.set_factor_grads(plan, gtot, self.Bcp)
            return loss_out[0].clone()

        def log_loss(ii):
            plan.loss_grad(Xd, yd, cw, W, plan.pack(self.Bcp), w, grad)  # data loss only (reference :372)
            loss = float(grad[plan.num_params].item())
            return loss, (_fit.line_plain(ii, loss) if verbose == 2 else None)

        return _fit.lbfgs_fit(self.Bcp, LBFGS_kwargs, closure_loss, log_loss, stop="index", max_iter=max_iter,
                              tol=tol, patience=patience, running_loss_logging_interval=running_loss_logging_interval,
                              verbose=verbose, loss_running=self.loss_running)

    def fit_Adam(self, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, weights=None, verbose=False,
                 Adam_kwargs=None, process_group=None):
        """Adam fit (multinomial_tensor_regression.py:389-471), device resident on gfx950.

        process_group: optional torch.distributed group; self.X / self.y are then this rank's
        sample shard (the CE normaliser sum_n w[y_n] is all-reduced once)."""
        hp = adam_hparams(Adam_kwargs)

        def prepare():
            dev, Xd, yd = self._device_data()
            plan = self._get_plan(Xd, Xd.shape[0])
            cw, W = self._class_weights(weights, dev, yd)
            return dev, Xd, yd, plan, cw, W
        if process_group is not None:
            # collectives first, then the rank-local checks with a collective verdict: a failure on
            # one rank raises on every rank instead of leaving the others in a later all-reduce
            self._sync_class_set(process_group)
        (dev, Xd, yd, plan, cw, _), W = _fit.start_adam(process_group, prepare, lambda o: o[5], lambda o: o[3])
        arena = plan.pack(self.Bcp)
        w = self.weights.to(f"cuda:{dev}", torch.float32).contiguous()
        vcb = _fit.VerbosePrinter(_fit.line_plain) if verbose == 2 else None
        convergence_reached, _ = run_adam_fit(plan, Xd, yd, cw, W, arena, w, lambda_L2, max_iter, tol, patience,
                                              hp, self.loss_running, verbose_cb=vcb, process_group=process_group,
                                              arena_checked=True)
        plan.unpack_into(arena, self.Bcp)
        return _fit.finish_fit(convergence_reached, verbose)

    def predict(self, X=None, y_true=None, Bcp=None, device=None):
        """(probabilities, argmax) as numpy (multinomial…py:474-545); the 'logit' the reference
        returns is the softmax output (quirk Q2)."""
        from .util import HostStream
        if device is None:
            device = self.device
        if X is None:
            X = self.X
        if isinstance(X, HostStream):  # chunk by chunk through the same forward kernel
            Bd = [torch.as_tensor(A).to(f"cuda:{X.dev_index}") for A in (self.Bcp if Bcp is None else Bcp)]
            logit = torch.cat([model(Xc, Bd, self.weights, self.non_negative, softplus_kwargs=self.softplus_kwargs)
                               for _, _, Xc in X.chunks()]).detach().cpu().numpy()
            return logit, np.argmax(logit, axis=1)
        X, Bcp = _fit.coerce_predict_inputs(X, Bcp, self.Bcp, device)
        dev = _engine.compute_device(X, device)
        Xd = _engine.as_device_rows(X, dev)
        logit = model(Xd, [torch.as_tensor(A).to(f"cuda:{dev}") for A in Bcp], self.weights, self.non_negative,
                      softplus_kwargs=self.softplus_kwargs).detach().cpu().numpy()
        pred = np.argmax(logit, axis=1)
        return logit, pred

    def return_Bcp_final(self):
        Bcp = list(non_neg_fn(self.Bcp, self.non_negative, softplus_kwargs=self.softplus_kwargs))
        return [Bcp[ii].detach().cpu().numpy() for ii in range(len(Bcp))]

    def make_confusion_matrix(self, prob_or_pred='pred', prob=None, pred=None, y_true=None):
        """(multinomial…py:562-597)"""
        if (prob is None) and (pred is None):
            prob, pred = self.predict()
        if y_true is None:
            y_true = self.y.detach().cpu().numpy()
        if prob_or_pred == 'pred':
            cm = confusion_matrix(pred, y_true)
        elif prob_or_pred == 'prob':
            cm = confusion_matrix(prob, y_true)
        acc = np.sum(np.diag(cm)) / np.sum(cm)
        return cm, acc

    def detach_Bcp(self):
        return [Bcp.detach().cpu().numpy() for Bcp in self.Bcp]

    def get_params(self):
        # the reference reads a nonexistent self.bias here (quirk Q4); the working subset is returned
        X = self.X.X if not isinstance(self.X, torch.Tensor) else self.X  # HostStream: its host tensor
        return {'X': X.detach().cpu().numpy(),
                'y': self.y.detach().cpu().numpy(),
                'weights': self.weights.detach().cpu().numpy(),
                'Bcp': self.detach_Bcp(),
                'non_negative': self.non_negative,
                'softplus_kwargs': self.softplus_kwargs,
                'rank': self.rank,
                'device': self.device,
                'loss_running': self.loss_running}

    def set_params(self, params):
        self.X = params['X']
        self.y = params['y']
        self.weights = params['weights']
        self.Bcp = params['Bcp']
        if 'bias' in params:
            self.bias = params['bias']
        self.non_negative = params['non_negative']
        self.softplus_kwargs = params['softplus_kwargs']
        self.rank = params['rank']
        self.device = params['device']
        self.loss_running = params['loss_running']
        self._plan = None
        self._dev_cache = None
        self._cw_cache = None

    def display_params(self):
        print('X:', self.X.shape)
        print('y:', self.y.shape)
        print('weights:', self.weights)
        print('Bcp:', self.Bcp)
        print('non_negative:', self.non_negative)
        print('softplus_kwargs:', self.softplus_kwargs)
        print('rank:', self.rank)
        print('device:', self.device)
        print('loss_running:', self.loss_running)

    def plot_outputs(self):
        plt = _fit.plot_loss(self.loss_running)
        logit, pred = self.predict()
        fig, axs = plt.subplots(2)
        axs[0].imshow(idx_to_oneHot(pred, self.n_classes), aspect='auto', interpolation='none')
        axs[1].imshow(idx_to_oneHot(self.y.detach().cpu().numpy(), self.n_classes), aspect='auto',
                      interpolation='none')
        axs[1].set_xlabel('class')
        fig.suptitle('predictions')
        cm, acc = self.make_confusion_matrix(prob_or_pred='pred')
        fig = plt.figure()
        plt.imshow(cm)
        plt.ylabel('true class')
        plt.xlabel('predicted class')
        plt.title('confusion matrix (predictions)')
        Bcp_final = self.return_Bcp_final()
        fig, axs = plt.subplots(len(Bcp_final))
        for ii, val in enumerate(Bcp_final):
            axs[ii].set_title(f'factor {ii}')
            axs[ii].plot(val)
        fig.suptitle('components')


####################################
######## Scoring a sweep ###########
####################################

def _is_host_stream(X):
    from .util import HostStream
    return isinstance(X, HostStream)


def _per_entry(name, value, M):
    """None, or a list with one entry per element of `models` (ValueError on another length)."""
    if value is None:
        return [None] * M
    if not isinstance(value, (list, tuple)):
        raise ValueError(f"{name} must be None or a list with one entry per model, got {type(value).__name__}")
    if len(value) != M:
        raise ValueError(f"{name}: a list must hold one entry per model ({M}), got {len(value)}")
    return list(value)


def _host_labels(y):
    """Labels that live on the host as an int64 ndarray; None for a tensor on a device."""
    if isinstance(y, torch.Tensor):
        return None if y.device.type != "cpu" else y.detach().to(torch.long).reshape(-1).numpy()
    return np.asarray(y).astype(np.int64).reshape(-1)


class _ScoreEntry:
    """One (model, data set) pair of predict_many / score_many."""
    __slots__ = ("j", "model", "X", "Bcp", "own_Bcp", "N", "dims", "C", "R", "y", "yh", "cw", "arena_at")


class _ScoreMember:
    """One member of _engine.run_score_many."""
    __slots__ = ("X", "y", "arena", "arena_at", "w", "cw", "n_classes", "rank", "nonneg", "beta", "thr")


def _score_entries(who, models, X, y_true, weights, Bcp, need_y):
    """One record per (model, data set) pair with every argument error of every entry raised.  Nothing
    here touches a device unless labels already live on one: their range is then read there, all such
    label tensors of the call in one reduction and one host sync (none for a model's own y that a fit
    or an earlier call has checked)."""
    M = len(models)
    Xs, ys, Bs = _per_entry("X", X, M), _per_entry("y_true", y_true, M), _per_entry("Bcp", Bcp, M)
    if weights is None or not isinstance(weights, (list, tuple)) or (
            len(weights) > 0 and np.ndim(weights[0]) == 0 and weights[0] is not None):
        cws = [weights] * M  # None, or one class-weight vector for every entry
    else:
        cws = _per_entry("weights", weights, M)
    entries = []
    own = {}       # id(model) -> (Bcp, dims, C, R) of a model's own factors
    labels = {}    # (id(y), C) -> (n, host labels or None), checked
    on_device = {}  # (C, device) -> [label tensors on a device, range not yet known]
    cw_seen = {}   # id(weights entry) -> checked host vector
    for j, m in enumerate(models):
        if not isinstance(m, CP_logistic_regression):
            raise TypeError(f"{who} takes CP_logistic_regression objects of the multinomial modules, "
                            f"got {type(m).__name__}")
        e = _ScoreEntry()
        e.j, e.model = j, m
        e.X = m.X if Xs[j] is None else Xs[j]
        e.own_Bcp = Bs[j] is None
        got = own.get(id(m)) if e.own_Bcp else None
        if got is None:
            B = list(m.Bcp if e.own_Bcp else Bs[j])  # (a list of its own: conversions stay out of the caller's)
            got = (B, [int(A.shape[0]) for A in B[:-1]], int(B[-1].shape[0]), int(B[0].shape[1]))
            if e.own_Bcp:
                own[id(m)] = got
        e.Bcp, e.dims, e.C, e.R = got
        K = len(e.dims)
        shape = [int(d) for d in e.X.shape]
        if len(shape) != K + 1 or shape[1:] != e.dims:
            raise ValueError(f"Incorrect shapes for inner product along {K} common modes. "
                             f"tensor_1.shape={shape}, factors={[tuple(A.shape) for A in e.Bcp]}")
        e.N = shape[0]
        if e.N < 1:
            raise ValueError(f"{who}: entry {j} has no samples")
        e.y = e.yh = e.cw = None
        if need_y:
            e.y = y = m.y if ys[j] is None else ys[j]
            seen = labels.get((id(y), e.C))
            if seen is None:
                yh = _host_labels(y)
                n_y = int(y.numel()) if yh is None else int(yh.size)
                if n_y > 0 and yh is not None:
                    ymin, ymax = int(yh.min()), int(yh.max())
                    if ymin < 0 or ymax >= e.C:
                        raise IndexError(f"Target {ymax if ymax >= e.C else ymin} is out of bounds.")
                elif n_y > 0:
                    c = m._dev_cache  # (_device_data has read the range of the model's own labels)
                    if not (y is m.y and e.own_Bcp and c is not None and c[2] is y):
                        on_device.setdefault((e.C, y.device), []).append(y)
                seen = labels[(id(y), e.C)] = (n_y, yh)
            if seen[0] != e.N:
                raise ValueError(f"{who}: entry {j} has {e.N} samples and {seen[0]} labels")
            e.yh = seen[1]
            if cws[j] is not None:
                cw = cw_seen.get(id(cws[j]))
                if cw is None:
                    cwh = torch.as_tensor(cws[j], dtype=torch.float32).detach().cpu()
                    if cwh.ndim != 1 or cwh.numel() != e.C:
                        raise RuntimeError(f"weight tensor should be defined either for all {e.C} classes or no "
                                           f"classes but got weight tensor of shape: {list(cwh.shape)}")
                    cw = cw_seen[id(cws[j])] = cwh.numpy()
                elif cw.size != e.C:
                    raise RuntimeError(f"weight tensor should be defined either for all {e.C} classes or no "
                                       f"classes but got weight tensor of shape: {list(cw.shape)}")
                e.cw = cw
        entries.append(e)
    for (C, _), group in on_device.items():
        yy = torch.cat([y.reshape(-1) for y in group])
        ymin, ymax = torch.stack((yy.min(), yy.max())).tolist()
        if ymin < 0 or ymax >= C:
            raise IndexError(f"Target {ymax if ymax >= C else ymin} is out of bounds.")
    return entries


def _score_route(entries, who):
    """(device index, indices scored in the batch, indices handled alone)."""
    devs, seen = set(), set()
    for e in entries:
        key = (id(e.X), id(e.model))
        if key not in seen:
            seen.add(key)
            devs.add(e.X.dev_index if _is_host_stream(e.X) else _engine.compute_device(e.X, e.model.device))
    if len(devs) != 1:
        raise ValueError(f"{who}: the models are on different devices ({sorted(devs)})")
    on = _engine.resident_enabled()
    batched, alone, inside = [], [], {}
    for e in entries:
        ok = False
        if on and len(e.dims) == 2 and not _is_host_stream(e.X):
            key = (e.dims[0], e.dims[1], e.C, e.R)
            ok = inside.get(key)
            if ok is None:
                ok = inside[key] = _engine.score_envelope(*key)
        (batched if ok else alone).append(e.j)
    return devs.pop(), batched, alone


def _score_members(entries, dev, need_y):
    """The batch's inputs on cuda:dev as run_score_many's members.  Tensors already there are used in
    place (X at its own row stride); what lives on the host goes up packed, one upload per kind, and an
    object that several entries share (one model's X, y or factors on four data sets) goes up once."""
    device = f"cuda:{dev}"

    def place(items, dtype, to_dev):
        """items: [(key, value)]; returns {key: device tensor}, host values through one packed upload."""
        out, host = {}, {}
        for key, v in items:
            if key in out or key in host:
                continue
            if isinstance(v, torch.Tensor) and v.device.type == "cuda":
                out[key] = to_dev(v)
            else:
                host[key] = v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        for key, t in zip(host, _engine.upload_packed(list(host.values()), dtype, dev)):
            out[key] = t
        return out

    for e in entries:
        if isinstance(e.X, torch.Tensor) and e.X.dtype != torch.float32:
            raise TypeError(f"the gfx950 path of this model computes in torch.float32; got X of dtype {e.X.dtype}")
    def rows_in_place(v):  # any base alignment will do: the kernel reads X with 4-byte loads
        v = v if v.device.index == dev else v.to(device)
        return v if _engine._rows_contiguous(v) else v.contiguous()

    Xd = place([(id(e.X), e.X) for e in entries], np.float32, rows_in_place)
    yd = place([(id(e.y), e.y) for e in entries if need_y], np.int64,
               lambda v: v if (v.dtype == torch.long and v.ndim == 1 and v.is_contiguous() and v.device.index == dev)
               else v.to(device, torch.long).reshape(-1).contiguous())
    cwd = place([(id(e.cw), e.cw) for e in entries if e.cw is not None], np.float32, None)
    wd = place([(id(e.model), e.model.weights) for e in entries], np.float32,
               lambda v: v.detach().to(device, torch.float32).reshape(-1).contiguous())
    # every distinct factor list in ONE arena, an offset per entry
    srcs, at, total = [], {}, 0
    for e in entries:
        key = id(e.model) if e.own_Bcp else ("entry", e.j)
        if key not in at:
            at[key] = total
            for f, A in enumerate(e.Bcp):
                A = A if isinstance(A, torch.Tensor) else torch.as_tensor(np.asarray(A), dtype=torch.float32)
                if tuple(A.shape) != ((e.dims + [e.C])[f], e.R):
                    raise ValueError(f"factor {f} has shape {tuple(A.shape)}, expected {((e.dims + [e.C])[f], e.R)}")
                srcs.append(A.detach().reshape(-1))
                total += srcs[-1].numel()
        e.arena_at = at[key]
    arena = _engine._pack_arena(srcs, total, torch.float32, device)
    members, nonlin = [], {}
    for e in entries:
        nl = nonlin.get(id(e.model))
        if nl is None:
            nl = nonlin[id(e.model)] = _engine.nonlin_key(e.model.non_negative, e.model.softplus_kwargs, 3)
            if wd[id(e.model)].numel() != e.R:
                raise ValueError(f"the CP component weights hold {wd[id(e.model)].numel()} values, the factors "
                                 f"have rank {e.R}")
        mb = _ScoreMember()
        mb.X, mb.y, mb.arena, mb.arena_at, mb.w = Xd[id(e.X)], yd[id(e.y)] if need_y else None, arena, e.arena_at, \
            wd[id(e.model)]
        mb.cw = None if e.cw is None else cwd[id(e.cw)]
        mb.n_classes, mb.rank, (mb.nonneg, mb.beta, mb.thr) = e.C, e.R, nl
        members.append(mb)
    return members


def _host_score(prob, pred, y, cw, C):
    """The metrics of one entry from predict's output, on the host: the double-softmax CrossEntropyLoss
    sums in float64 and counts[pred, true]."""
    S = np.asarray(prob, dtype=np.float64)
    S = S - S.max(axis=1, keepdims=True)
    l = -(S[np.arange(y.size), y] - np.log(np.exp(S).sum(axis=1)))
    w = np.ones(y.size) if cw is None else np.asarray(cw, dtype=np.float64)[y]
    counts = np.zeros((C, C), dtype=np.int64)
    np.add.at(counts, (pred, y), 1)
    return float((w * l).sum()), float(w.sum()), counts


def _alone_predict(e):
    return e.model.predict(X=e.X, Bcp=None if e.own_Bcp else list(e.Bcp))


def predict_many(models, X=None, Bcp=None, report=None):
    """`models[j].predict(X=X[j], Bcp=Bcp[j])` of many (model, data set) pairs in one launch: returns
    [(prob (N_j, C_j) float32 ndarray, pred (N_j,) int64 ndarray)].

    models: CP_logistic_regression objects of either multinomial module; the same object may appear
    several times (one model on several data sets).  X and Bcp are None (each model's own) or lists
    with one entry per model, an entry itself None, an ndarray or a tensor (Bcp: a list of factors).
    An entry inside the kernel's envelope (3-D X, n_classes and rank <= 16, the dense coefficient
    tensor within one CU's LDS; TR_MNL_RESIDENT not 0) is scored in the batch, every other by its own
    `predict`.  report (a dict) receives {'batched': indices, 'alone': indices, 'launches': n}."""
    models = list(models)
    _many.start_report(report, batched=[], alone=[], launches=0)
    if not models:
        return []
    entries = _score_entries("predict_many", models, X, None, None, Bcp, need_y=False)
    dev, batched, alone = _score_route(entries, "predict_many")
    results = [None] * len(models)
    if batched:
        got = _engine.run_score_many(dev, _score_members([entries[j] for j in batched], dev, False), "predict")
        for j, r in zip(batched, got):
            results[j] = r
    for j in alone:
        results[j] = _alone_predict(entries[j])
    return _many.finish_many(results, False, report, batched=batched, alone=alone, launches=1 if batched else 0)


def score_many(models, X=None, y_true=None, weights=None, report=None):
    """What a hyperparameter grid keeps of every (model, data set) pair, in one launch: returns
    [{'loss': float, 'acc': float, 'counts': (C, C) int64 ndarray [pred, true], 'cm': ndarray}].

    'loss' is sum w[y] l / sum w[y], the data loss fit_Adam records for that model on that data (the
    CrossEntropyLoss of the softmax output); weights is None (unweighted), one class-weight vector for
    all entries or a list of one per entry.  'acc' is trace(counts) / N and 'cm' the column-normalised
    counts, `confusion_matrix(pred, y)` of this module.  models, X and report as in predict_many;
    y_true like X (None: each model's own y).  Only the loss sums and the integer counts come back from
    the device, in one packed copy; no probabilities are downloaded."""
    models = list(models)
    _many.start_report(report, batched=[], alone=[], launches=0)
    if not models:
        return []
    entries = _score_entries("score_many", models, X, y_true, weights, None, need_y=True)
    dev, batched, alone = _score_route(entries, "score_many")
    raw = [None] * len(models)
    if batched:
        got = _engine.run_score_many(dev, _score_members([entries[j] for j in batched], dev, True), "score")
        for j, r in zip(batched, got):
            raw[j] = r
    for j in alone:
        e = entries[j]
        prob, pred = _alone_predict(e)
        yh = e.yh if e.yh is not None else e.y.detach().cpu().numpy().reshape(-1)
        raw[j] = _host_score(prob, pred, yh, e.cw, e.C)
    results = []
    with np.errstate(divide="ignore", invalid="ignore"):  # (a class absent from y: its column is 0 / 0, as the module's)
        for e, (lsum, wsum, counts) in zip(entries, raw):
            results.append({"loss": lsum / wsum, "acc": float(np.trace(counts) / e.N), "counts": counts,
                            "cm": counts / np.sum(counts, axis=0)[None, :]})
    return _many.finish_many(results, False, report, batched=batched, alone=alone, launches=1 if batched else 0)


####################################
####### Many models, one X #########
####################################

# The smallest group the shared-X sweep takes, by the largest class count in the group: a group reads X
# twice per iteration and runs its GEMMs in exact fp32 on the matrix cores, a model alone reads X once
# where its single-pass kernel applies.  Measured against the loop of fit_Adam calls (tools/
# mnl_many_shapes.py, DESIGN.md "Shared-X multinomial sweep"); per class count the smallest measured M
# that beats the loop at every measured shape by more than the spreads, an unmeasured class count takes
# the threshold of the next larger measured one, and None keeps a class count with the loop.  From
# profiles/mnl_many_shapes.txt (ms per iteration, group against loop):
#   C = 5   M = 1: 0.958 / 1.304 (line 7, the notebook shape) but 0.837 / 0.423 (line 16, config 3's shape);
#           M = 2: 0.827 / 0.811 (line 17) loses; M = 3: 1.036 / 3.882 (line 9) and 0.846 / 1.192 (line 18)   -> 3
#   C = 10  M = 2: 1.034 / 0.814 (line 12) loses; M = 3: 1.063 / 1.186 (line 13), spreads 0.006 + 0.036  -> 3
#   C = 16  M = 4: 2.183 / 10.251 (line 15, the notebook shape) but 1.758 / 1.606 (line 22, config 3's
#           shape): never ahead at every measured shape                                                 -> None
MNL_MANY_MIN_BATCH = {5: 3, 10: 3, 16: None}


def mnl_many_min_batch(n_classes):
    """The default minimum group size for a group whose largest class count is `n_classes` (None: the
    loop of fit_Adam calls is never slower; such a group is formed only with an explicit min_batch)."""
    for C in sorted(MNL_MANY_MIN_BATCH):
        if n_classes <= C:
            return MNL_MANY_MIN_BATCH[C]
    return None


def _x_key(Xd):
    """Two models share a stream when their device X is the same storage seen the same way."""
    return (Xd.data_ptr(), tuple(Xd.shape), tuple(Xd.stride()), Xd.dtype, str(Xd.device))


def fit_Adam_many(models, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, weights=None, verbose=False,
                  Adam_kwargs=None, min_batch=None, report=None):
    """fit_Adam of many CP_logistic_regression models that share ONE X: the outer loop of a
    hyperparameter grid (demo_MultinomialTensorRegression.ipynb: a fresh model per grid point, every
    model on the same X) with X streamed twice per iteration for a whole group of models instead of
    once per model.

    models: CP_logistic_regression objects of this module, each with its own y, class count, rank,
    non_negative, softplus_kwargs, CP weights, initial Bcp and loss_running.  lambda_L2, max_iter, tol,
    patience, weights (class weights, as in fit_Adam) and Adam_kwargs are each one value for all models
    or a list of len(models) values.  Afterwards every model is in the state its own `fit_Adam(...)`
    would have left it, up to fp32 summation order (Bcp, loss_running extended, plateau stops included);
    `model._plan` is untouched.  The returned list holds each model's convergence_reached.

    Models whose device X is the same storage (data pointer, shape, strides, dtype) share a stream:
    that is what happens when every model was built from one float32 device tensor.  Building each
    model from a numpy X uploads a private copy per model, and those models do not group.  Within one
    X, groups are filled in list order while the class counts sum to at most 64 columns (12 models at
    5 classes); labels and class counts may differ per model.  The envelope: float32, 3-D X, 2..16
    classes, rank <= 32, P = I * J and X's row stride multiples of 4 floats (a windowed or padded
    stride included), X 16-byte aligned, any N >= 1.  A group of fewer than `min_batch` models (None:
    mnl_many_min_batch of its largest class count, measured) and every model outside the envelope go to
    their own fit_Adam, as do a 4-D X, a util.HostStream, an instance of the hierarchical subclass
    and every model under TR_MNL_MANY=0.  report (a dict) receives {'batched': indices, 'alone':
    indices, 'groups': n, 'x_passes': n}.  verbose=2 and process_group are not offered."""
    from .util import HostStream
    models = list(models)
    M = len(models)
    _many.check_models(models, CP_logistic_regression, verbose, " of every model")
    given = dict(lambda_L2=lambda_L2, max_iter=max_iter, tol=tol, patience=patience, Adam_kwargs=Adam_kwargs)
    args = {k: _many.per_member(k, v, M) for k, v in given.items()}
    # one class-weight vector is itself a sequence: only a list of sequences (or None) is per model
    cws = _many.per_member("weights", weights, M,
                           one_value=lambda v: len(v) > 0 and all(e is not None and np.ndim(e) == 0 for e in v))
    if min_batch is not None and int(min_batch) < 1:
        raise ValueError(f"min_batch must be >= 1, got {min_batch}")
    _many.start_report(report, batched=[], alone=[], groups=0, x_passes=0)
    if M == 0:
        return []
    hps = [adam_hparams(ak) for ak in args["Adam_kwargs"]]  # TypeError on None, as fit_Adam
    # ---- routing ----
    by_x, data = {}, {}
    if _engine.mnl_many_enabled():
        for j, m in enumerate(models):
            if type(m) is not CP_logistic_regression or isinstance(m.X, HostStream):
                continue
            if not isinstance(m.X, torch.Tensor) or m.X.ndim != 3 or m.X.dtype != torch.float32 or len(m.Bcp) != 3:
                continue
            dev, Xd, yd = m._device_data()
            N, I0, I1 = (int(d) for d in Xd.shape)
            C, R = int(m.Bcp[-1].shape[0]), int(m.Bcp[0].shape[1])
            xld = int(Xd.stride(0)) if N > 1 else I0 * I1
            if Xd.data_ptr() % 16 != 0 or not _engine.mnl_many_envelope(I0, I1, xld, C, R):
                continue
            data[j] = (dev, Xd, yd, C, R)
            by_x.setdefault(_x_key(Xd), []).append(j)
    groups = []
    for js in by_x.values():
        cur, cols = [], 0
        for j in js:
            if cols + data[j][3] > _engine.MNL_MANY_MAX_COLS:
                groups.append(cur)
                cur, cols = [], 0
            cur.append(j)
            cols += data[j][3]
        groups.append(cur)

    def big_enough(g):
        need = min_batch if min_batch is not None else mnl_many_min_batch(max(data[j][3] for j in g))
        return need is not None and len(g) >= int(need)
    groups = [g for g in groups if big_enough(g)]
    batched = sorted(j for g in groups for j in g)
    alone = [j for j in range(M) if j not in set(batched)]
    results, passes = [False] * M, 0
    for g in groups:
        dev, Xd = data[g[0]][0], data[g[0]][1]
        I0, I1 = int(Xd.shape[1]), int(Xd.shape[2])
        members, params = [], []
        for j in g:
            m = models[j]
            _, _, yd, C, R = data[j]
            nn, beta, thr = _engine.nonlin_key(m.non_negative, m.softplus_kwargs, 3)
            factors = [torch.as_tensor(A) for A in m.Bcp]
            for f, A in enumerate(factors):
                if tuple(A.shape) != ((I0, I1, C)[f], R):
                    raise ValueError(f"model {j}: factor {f} has shape {tuple(A.shape)}, expected {((I0, I1, C)[f], R)}")
            params.append(factors)
            cw, W = m._class_weights(cws[j], dev, yd)
            w = torch.as_tensor(m.weights).to(Xd.device, torch.float32).contiguous()
            if w.numel() != R:
                raise ValueError(f"model {j}: weights holds {w.numel()} values, the rank is {R}")
            members.append(types.SimpleNamespace(
                y=yd, w=w, cw=cw, W=W, n_classes=C, rank=R, nonneg=nn, beta=beta, thr=thr,
                lambda_L2=args["lambda_L2"][j], hp=hps[j], max_iter=args["max_iter"][j], tol=args["tol"][j],
                patience=args["patience"][j], loss_running=m.loss_running))
        arena, offsets, slices = _many.pack_members(params, Xd.device)
        for mb, own in zip(members, slices):
            mb.arena = own
        stops, n_pass = _engine.run_mnl_many(dev, Xd, members)
        passes += n_pass
        _many.unpack_members(arena, offsets, [tuple(models[j].Bcp) for j in g])
        for j, s in zip(g, stops):
            results[j] = s > 0
    for j in alone:  # outside the envelope, a small group or the route switched off: the model's own fit
        kw = {k: v[j] for k, v in args.items()}
        if type(models[j]) is CP_logistic_regression or cws[j] is not None:
            kw["weights"] = cws[j]
        results[j] = models[j].fit_Adam(verbose=False, **kw)
    return _many.finish_many(results, verbose, report, batched=batched, alone=alone, groups=len(groups),
                             x_passes=passes)
