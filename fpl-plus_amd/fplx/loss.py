"""Segmentation losses behind the reference's SegLossDict surface
(reference: PyMIC/pymic/loss/loss_dict_seg.py:31-41; classes loss/seg/dice.py:9-57 DiceLoss,
dice.py:95-128 DiceLoss_weight, loss/seg/ce.py:9-44 CrossEntropyLoss, loss/seg/combined.py:8-39
CombinedLoss; base class loss/seg/abstract.py:7-37; the second family - dice.py:130-199 FocalDiceLoss /
NoiseRobustDiceLoss, exp_log.py ExpLogLoss, ce.py:46-93 GeneralizedCELoss, mse.py MSELoss / MAELoss,
slsr.py SLSRLoss - registered in SegLossDictAll).

Same construction (`params` dict, `loss_softmax` key) and same call: forward(loss_input_dict) with
keys 'prediction', 'ground_truth', optional 'pixel_weight' [N,1,D,H,W] and 'image_weight' [N];
returns a scalar tensor that supports .backward().  One fused HIP pass evaluates softmax, every
requested term and the hard-Dice train metric; there is no CPU path.
"""
import torch
import torch.nn as nn

from . import ops


class _FusedSegLoss(torch.autograd.Function):
    """one ops.LossPass (either family) as an autograd node"""

    @staticmethod
    def forward(ctx, logits, label, pw, iw, lp, holder):
        logits, label, pw, iw = prepare_inputs(lp, logits, label, pw, iw)
        n, c = logits.shape[0], logits.shape[1]
        k, nout, ncoef = lp.sizes(n, c)
        dev = logits.device
        part = torch.empty((n, ops.loss_rows(logits[0, 0].numel()), k), dtype=torch.float32, device=dev)
        out = torch.empty(nout, dtype=torch.float32, device=dev)
        coef = torch.empty(ncoef, dtype=torch.float32, device=dev)
        lp.forward(logits, label, pw, iw, part, out, coef, getattr(holder, "dist_group", None), getattr(holder, "dist_sync", False))
        ctx.save_for_backward(logits, label, pw, coef)
        ctx.lp = lp
        if holder is not None:
            holder.last_out = out
        return out[0]

    @staticmethod
    def backward(ctx, g):
        logits, label, pw, coef = ctx.saved_tensors
        dl = torch.empty_like(logits)
        ctx.lp.backward(logits, label, pw, coef, g.float().contiguous(), dl)
        return dl, None, None, None, None, None


def ext_spec(ext, ext_params):
    """(weights, parameters) of the second family's terms in the order of ops.LOSS_EXT_TERMS / LOSS_EXT_PARAMS - hashable;
    None when no such term is asked for"""
    if not any(float(t) != 0.0 for t in ext):
        return None
    prm = [ext_params.get(k, d) for k, d in zip(ops.LOSS_EXT_PARAMS, ops.LOSS_EXT_DEFAULTS)]
    prm[6] = bool(prm[6])
    prm[7] = None if prm[7] is None else tuple(float(t) for t in prm[7])
    return tuple(float(t) for t in ext), tuple(float(t) for t in prm[:6]) + (prm[6], prm[7])


def check_ext_inputs(spec, pw):
    """what the reference raises before it computes (ce.py:85-88)"""
    if spec is not None and spec[0][ops.LOSS_EXT_TERMS.index("gce")] != 0.0 and spec[1][6] and pw is None:
        raise ValueError("Pixel weight is enabled but not defined")


def prepare_inputs(lp, logits, label, pw, iw):
    """the checks every route into the pass `lp` (ops.LossPass) makes, and fp32 contiguous tensors -> (logits, label, pw, iw)"""
    if lp.terms[2] != 0.0 and (pw is None or iw is None):
        raise KeyError('pixel_weight')                                   # dice.py:109-110 index the dict
    if lp.terms[2] == 0.0:
        iw = None
    check_ext_inputs(lp.ext, pw)
    ops.require_gpu(logits, label, pw, iw)
    if logits.dim() != 5:
        raise ValueError("{0:}D tensor not supported".format(logits.dim()))        # loss/seg/util.py:46-47
    if logits.shape != label.shape:
        raise ValueError("fplx loss: prediction {0:} and ground_truth {1:} differ in shape".format(
            tuple(logits.shape), tuple(label.shape)))
    logits, label = logits.float().contiguous(), label.float().contiguous()
    if pw is not None:
        pw = pw.float().contiguous()
        if pw.numel() != logits.numel() // logits.shape[1]:
            raise ValueError("fplx loss: pixel_weight must be [N,1,D,H,W]")
    if iw is not None:
        iw = iw.float().contiguous()
    return logits, label, pw, iw


class AbstractSegLoss(nn.Module):
    """loss/seg/abstract.py:7-21.  `terms` = weights of (Dice, CE, image-weighted Dice, entropy); `ext` = weights of the second
    family's terms (ops.LOSS_EXT_TERMS), `ext_params` = their parameters (ops.LOSS_EXT_PARAMS; one slot per loss)."""
    terms = (0.0, 0.0, 0.0, 0.0)
    ext = (0.0,) * len(ops.LOSS_EXT_TERMS)
    ext_params = {}
    needs_weights = False

    def __init__(self, params=None):
        super(AbstractSegLoss, self).__init__()
        self.softmax = True if params is None else params.get('loss_softmax', True)
        self.last_out = None      # device tensor [4 + C]: total, dice, ce, entropy, hard class Dice[C]; with terms of the second
        # family [4 + C + 7]: behind these the values of ops.LOSS_EXT_TERMS
        # data parallelism (fplx.ddp.attach): evaluate the loss over the FULL batch of all ranks, as the reference's
        # nn.DataParallel does on its gathered logits; the ranks' gradients then add up to the full-batch gradient
        self.dist_sync, self.dist_group = False, None

    def _run(self, loss_input_dict, terms):
        predict = loss_input_dict['prediction']
        if isinstance(predict, (list, tuple)):
            predict = predict[0]                                             # dice.py:26-27
        lp = ops.LossPass(terms, self.ext_spec(), self.softmax)
        return _FusedSegLoss.apply(predict, loss_input_dict['ground_truth'], loss_input_dict.get('pixel_weight', None),
                                   loss_input_dict.get('image_weight', None), lp, self)

    def ext_spec(self):
        return ext_spec(self.ext, self.ext_params)

    def forward(self, loss_input_dict):
        return self._run(loss_input_dict, self.terms)


class DiceLoss(AbstractSegLoss):
    terms = (1.0, 0.0, 0.0, 0.0)


class CrossEntropyLoss(AbstractSegLoss):
    terms = (0.0, 1.0, 0.0, 0.0)


class DiceLoss_weight(AbstractSegLoss):
    terms = (0.0, 0.0, 1.0, 0.0)
    needs_weights = True


class EntropyTerm(AbstractSegLoss):
    """the regulariser SegmentationAgent.training adds (net_run_dsbn/agent_seg.py:352-354)"""
    terms = (0.0, 0.0, 0.0, 1.0)


def _one_hot_ext(name):
    return tuple(1.0 if t == name else 0.0 for t in ops.LOSS_EXT_TERMS)


class FocalDiceLoss(AbstractSegLoss):
    """dice.py:130-161; `focaldiceloss_beta` (>= 1)"""
    ext = _one_hot_ext("focal")

    def __init__(self, params=None):
        super(FocalDiceLoss, self).__init__(params)
        self.beta = params['FocalDiceLoss_beta'.lower()]
        self.ext_params = {"beta": float(self.beta)}


class NoiseRobustDiceLoss(AbstractSegLoss):
    """dice.py:163-199; `noiserobustdiceloss_gamma` (documented as (1, 2), not enforced)"""
    ext = _one_hot_ext("noise_robust")

    def __init__(self, params):
        super(NoiseRobustDiceLoss, self).__init__(params)
        self.gamma = params['NoiseRobustDiceLoss_gamma'.lower()]
        self.ext_params = {"gamma_nr": float(self.gamma)}


class ExpLogLoss(AbstractSegLoss):
    """exp_log.py:10-56; `explogloss_w_dice` in [0, 1] and `explogloss_gamma`"""
    ext = _one_hot_ext("explog")

    def __init__(self, params):
        super(ExpLogLoss, self).__init__(params)
        self.w_dice = params['ExpLogLoss_w_dice'.lower()]
        self.gamma = params['ExpLogLoss_gamma'.lower()]
        self.ext_params = {"w_dice_el": float(self.w_dice), "gamma_el": float(self.gamma)}


class GeneralizedCELoss(AbstractSegLoss):
    """ce.py:46-93 as DOCUMENTED there: `loss_gce_q`, `loss_with_pixel_weight` (the weighted mean
    sum(gce w) / sum(w)), `loss_class_weight` (gce_c x weight_c)"""
    ext = _one_hot_ext("gce")

    def __init__(self, params):
        super(GeneralizedCELoss, self).__init__(params)
        self.q = params.get('loss_gce_q', 0.5)
        self.enable_pix_weight = params.get('loss_with_pixel_weight', False)
        self.cls_weight = params.get('loss_class_weight', None)
        self.ext_params = {"q": float(self.q), "use_pixel_weight": bool(self.enable_pix_weight),
                           "class_weight": None if self.cls_weight is None else tuple(float(t) for t in self.cls_weight)}


class MAELoss(AbstractSegLoss):
    """mse.py:29-50"""
    ext = _one_hot_ext("mae")


class MSELoss(AbstractSegLoss):
    """mse.py:5-26"""
    ext = _one_hot_ext("mse")


class SLSRLoss(AbstractSegLoss):
    """slsr.py:10-58; `slsrloss_epsilon` (default 0.25); pixel_weight is the mask of unconfident voxels (> 0)"""
    ext = _one_hot_ext("slsr")

    def __init__(self, params=None):
        super(SLSRLoss, self).__init__(params)
        if params is None:
            params = {}
        self.epsilon = params.get('slsrloss_epsilon', 0.25)
        self.ext_params = {"epsilon": float(self.epsilon)}


SegLossDict = {
    'DiceLoss': DiceLoss,
    'CrossEntropyLoss': CrossEntropyLoss,
    'DiceLoss_weight': DiceLoss_weight,
}

# the reference's nine names (loss/loss_dict_seg.py:31-41) plus DiceLoss_weight: what SegmentationAgent uses when no dictionary
# was set.  SegLossDict stays the three names of the first family (why two).
SegLossDictAll = dict(SegLossDict)
SegLossDictAll.update({
    'GeneralizedCELoss': GeneralizedCELoss,
    'FocalDiceLoss': FocalDiceLoss,
    'NoiseRobustDiceLoss': NoiseRobustDiceLoss,
    'ExpLogLoss': ExpLogLoss,
    'MAELoss': MAELoss,
    'MSELoss': MSELoss,
    'SLSRLoss': SLSRLoss,
})


class CombinedLoss(AbstractSegLoss):
    """loss/seg/combined.py:20-39: weighted sum of registered losses - evaluated in ONE pass."""

    def __init__(self, params, loss_dict, extra_entropy=0.0):
        super(CombinedLoss, self).__init__(params)
        loss_names = params['loss_type']
        self.loss_weight = params['loss_weight']
        assert (len(loss_names) == len(self.loss_weight))
        terms = [0.0, 0.0, 0.0, float(extra_entropy)]
        ext, ext_params = [0.0] * len(ops.LOSS_EXT_TERMS), {}
        for name, w in zip(loss_names, self.loss_weight):
            if name not in loss_dict:
                raise ValueError("{0:} is not defined, or has not been added to the \
                    loss dictionary".format(name))
            cls = loss_dict[name]
            if not (isinstance(cls, type) and issubclass(cls, AbstractSegLoss)):
                raise ValueError("fplx CombinedLoss fuses fplx losses only; {0:} is foreign".format(name))
            for i, t in enumerate(cls.terms):
                terms[i] += w * t
            if any(t != 0.0 for t in cls.ext):
                sub = cls(params)                        # reads (and demands) its keys as the reference's constructor does
                for i, t in enumerate(sub.ext):
                    ext[i] += w * t
                for k, val in sub.ext_params.items():
                    if k in ext_params and ext_params[k] != val:
                        raise ValueError("fplx CombinedLoss: {0:} asks for {1:} = {2:} but another term set {3:}; there is one "
                                         "parameter slot per loss".format(name, k, val, ext_params[k]))
                    ext_params[k] = val
        self.terms = tuple(terms)
        self.ext, self.ext_params = tuple(ext), ext_params


class DeepSuperviseLoss(AbstractSegLoss):
    """loss/seg/deep_sup.py:7-41: the base loss once per output scale of a deep-supervised network on the shared ground truth and
    weights, sum_i w_i loss_i / sum_i w_i.  `base_loss` is an fplx loss (one fused pass per scale).  The weights are read from
    `deep_suervise_weight` (sic, deep_sup.py:21); the reference's agent passes `deep_supervise_weight` (agent_seg.py:126-129),
    so through the agent they are always [1.0] * outputs - reproduced.  Not in SegLossDictAll, as in the reference.
    `last_out` is the base loss's of output 0: the agent's train-time class Dice comes from the full-resolution output."""

    def __init__(self, params):
        super(DeepSuperviseLoss, self).__init__(params)
        self.deep_sup_weight = params.get('deep_suervise_weight', None)
        self.base_loss = params['base_loss']

    @property
    def dist_sync(self):
        return self.__dict__.get('_dist_sync', False)

    @dist_sync.setter
    def dist_sync(self, on):                       # the full-batch evaluation is the base loss's business
        self.__dict__['_dist_sync'] = on
        base = self.__dict__.get('_modules', {}).get('base_loss')
        if base is not None and hasattr(base, 'dist_sync'):
            base.dist_sync = on

    def forward(self, loss_input_dict):
        predict = loss_input_dict['prediction']
        if not isinstance(predict, (list, tuple)):
            raise ValueError("""For deep supervision, the prediction should
                be a list or a tuple""")
        predict_num = len(predict)
        if self.deep_sup_weight is None:
            self.deep_sup_weight = [1.0] * predict_num
        else:
            assert (predict_num == len(self.deep_sup_weight))
        loss_sum, weight_sum, first_out = 0.0, 0.0, None
        scale = dict(loss_input_dict)
        for i in range(predict_num):
            scale['prediction'] = predict[i]
            temp_loss = self.base_loss(scale)
            if i == 0:
                first_out = getattr(self.base_loss, 'last_out', None)
            loss_sum = loss_sum + temp_loss * self.deep_sup_weight[i]
            weight_sum += self.deep_sup_weight[i]
        self.last_out = first_out
        return loss_sum / weight_sum


def make_loss(training_cfg, loss_dict=None, entropy_weight=0.0):
    """create_loss_calculator (net_run_dsbn/agent_seg.py:113-132) for the fused losses."""
    loss_dict = SegLossDict if loss_dict is None else loss_dict
    name = training_cfg['loss_type']
    if isinstance(name, (list, tuple)):
        return CombinedLoss(training_cfg, loss_dict, entropy_weight)
    if name not in loss_dict:
        raise ValueError("Undefined loss function {0:}".format(name))          # agent_seg.py:120-121
    if entropy_weight == 0.0:
        return loss_dict[name](training_cfg)
    cfg = dict(training_cfg)
    cfg['loss_type'], cfg['loss_weight'] = [name], [1.0]
    return CombinedLoss(cfg, loss_dict, entropy_weight)
