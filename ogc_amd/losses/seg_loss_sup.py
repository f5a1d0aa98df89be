"""The supervised mask loss: Hungarian matching of predicted and GT objects by a cross-entropy (or focal) + Dice cost, then
the same two terms on the matched pairs.  Reference: losses/seg_loss_sup.py (names and signatures kept).

Two paths, chosen per call as in seg_loss_unsup.py:

  tensor path   the reference's formula restated without its two (B, N, K, K) repeats: the pairwise tables are formed one GT
                column at a time with the reference's own element-wise arithmetic, the labels are permuted by a gather.  Used on
                the CPU, and on the GPU for inputs the kernels do not take (not float32, not contiguous, K > 32).
  kernel path   on a float32 GPU tensor: ogc_sup_match_cost, ogc_lsap_maximize, ogc_sup_mask_loss_fwd and, in backward,
                ogc_sup_mask_loss_bwd (csrc/sup_loss.hip).  No (B, N, K, K) tensor, no permuted labels, no host round trip.

The assignment in both minimises  w_ce * cost_ce + w_dice * mean(cost_dice).

A quirk of the reference, kept: DiceLoss.match_cost ends in ``loss.mean()`` without an axis (:128), so the Dice part of the
matching cost is ONE scalar, the mean over the whole (B, K, K) table, added to every entry of every sample.  It cannot change
which assignment is cheapest; it can change which of several equally cheap ones (empty GT columns are identical) scipy's
tie-break returns, which leaves the permuted labels, the loss and the gradient unchanged.

A known deviation: the reference raises ValueError (from scipy) when the cost holds a NaN.  Here the sample's assignment
becomes -1, the loss NaN and so do the gradients, and the trainer's NaN rule skips the step.  (That is the kernel path, whose
element function turns a mask entry that is NaN or outside [0, 1] into NaN.  On the tensor path torch's
binary_cross_entropy refuses such an entry itself, as it does in the reference; a NaN that enters through the labels or
`valid` takes the route described here on both paths.)
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment

KERNELS = True   # cleared by tools/sup_loss_time.py and the GPU tests to run the tensor path on GPU tensors


def _weighted(loss, valid):
    if valid is not None:
        loss = loss * valid.reshape(valid.shape + (1,) * (loss.dim() - valid.dim()))
    return loss


class CrossEntropyLoss(nn.Module):
    """Reference: :8-38."""
    focal = None   # (alpha, gamma) of the kernels' element function; None = plain BCE

    def elementwise(self, pred, target):
        return F.binary_cross_entropy(pred, target, reduction='none')

    def forward(self, pred, target, valid=None):
        """pred, target (B, N, K), valid (B, N) or None -> () loss."""
        return _weighted(self.elementwise(pred, target), valid).mean()

    def match_cost(self, pred, target, valid=None):
        """pred, target (B, N, K, K), valid (B, N) or None -> (B, K, K)."""
        return _weighted(self.elementwise(pred, target), valid).mean(1)


class FocalLoss(CrossEntropyLoss):
    """Reference: :41-87."""

    def __init__(self, alpha=0.25, gamma=2):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma

    @property
    def focal(self):
        return (self.alpha, self.gamma)

    def elementwise(self, pred, target):
        ce_loss = F.binary_cross_entropy(pred, target, reduction='none')
        p_t = target * pred + (1 - target) * (1 - pred)
        loss = ce_loss * ((1 - p_t) ** self.gamma)
        if self.alpha >= 0:
            alpha_t = self.alpha * target + (1 - self.alpha) * (1 - target)
            loss = alpha_t * loss
        return loss


class DiceLoss(nn.Module):
    """Reference: :90-128."""

    def per_object(self, pred, target, valid=None):
        """1 - (2 sum p t v + 1) / (sum p v + sum t v + 1), summed over dim 1 (the points)."""
        if valid is not None:
            numerator = _weighted(2 * (pred * target), valid).sum(1)
            denominator = _weighted(pred, valid).sum(1) + _weighted(target, valid).sum(1)
        else:
            numerator = 2 * (pred * target).sum(1)
            denominator = pred.sum(1) + target.sum(1)
        return 1 - (numerator + 1) / (denominator + 1)

    def forward(self, pred, target, valid=None):
        """pred, target (B, N, K), valid (B, N) or None -> () loss."""
        return self.per_object(pred, target, valid).mean()

    def match_cost(self, pred, target, valid=None):
        """pred, target (B, N, K, K) -> a SCALAR: the reference takes the mean over the whole table (:128; module docstring)."""
        return self.per_object(pred, target, valid).mean()


def match_cost_tables(ce_loss, dice_loss, mask, gt_mask, valid=None):
    """(cost_ce, cost_dice), both (B, K, K) with rows = predicted slots and columns = GT slots: what ce_loss.match_cost and
    dice_loss.per_object give on the reference's (B, N, K, K) repeats, formed one GT column at a time."""
    mask = mask.detach()
    ce, dice = [], []
    for j in range(gt_mask.shape[-1]):
        t = gt_mask[:, :, j:j + 1].expand_as(mask)
        ce.append(_weighted(ce_loss.elementwise(mask, t), valid).mean(1))
        dice.append(dice_loss.per_object(mask, t, valid))
    return torch.stack(ce, 2), torch.stack(dice, 2)


def _columns_by_cost(cost):
    """(B, K, K) cost -> (B, K) int64: the GT column assigned to every predicted slot, scipy's
    linear_sum_assignment(cost, maximize=False) including its tie-break; all -1 for a sample whose cost holds a NaN.  On a
    float32 GPU tensor one launch of ogc_lsap_maximize on the negated cost (scipy's maximize=True is itself a negation)."""
    cost = cost.detach()
    n_batch, _, n_object = cost.shape
    if cost.is_cuda and n_object <= 64:
        from .. import pointnet2_cuda as nat
        cols = torch.empty((n_batch, n_object), dtype=torch.int32, device=cost.device)
        nat.lsap_maximize_wrapper(n_batch, n_object, (-cost).float().contiguous(), cols)
        return cols.long()
    cols = []
    for cost_b in cost.cpu().numpy():
        if np.isnan(cost_b).any():
            cols.append(np.full(n_object, -1, dtype=np.int64))
        else:
            cols.append(linear_sum_assignment(cost_b, maximize=False)[1].astype(np.int64))
    return torch.from_numpy(np.stack(cols, 0)).to(cost.device)


def match_mask_by_cost(cost):
    """(B, K, K) cost -> (B, K, K) float32 one-hot permutation minimising it (reference: :131-145).  A sample without an
    assignment (NaN cost) gets a NaN matrix."""
    cols = _columns_by_cost(cost)
    perm = torch.eye(cost.shape[-1], dtype=torch.float32, device=cost.device)[cols.clamp(min=0)]
    return torch.where((cols < 0)[..., None], torch.full_like(perm, float('nan')), perm)


def permute_labels(gt_mask, cols):
    """einsum('bij,bnj->bni', eye[cols], gt_mask) as a gather; NaN where cols is -1."""
    index = cols.clamp(min=0)[:, None, :].expand(gt_mask.shape)
    out = torch.gather(gt_mask, 2, index)
    return torch.where((cols < 0)[:, None, :], torch.full_like(out, float('nan')), out).detach()


class _FusedMaskLoss(torch.autograd.Function):
    """(loss, terms, cols) over the kernels; terms = [l_ce, l_dice] and cols (B, K) i32 carry no gradient."""

    @staticmethod
    def forward(ctx, mask, gt_mask, valid, focal, w_ce, w_dice):
        from .. import pointnet2_cuda as nat
        b, n, k = mask.shape
        dev = mask.device
        ws = nat.sup_loss_workspace(b, n, k, dev)
        cost_ce = torch.empty((b, k, k), dtype=torch.float32, device=dev)
        cost_dice = torch.empty((b, k, k), dtype=torch.float32, device=dev)
        nat.sup_match_cost_wrapper(b, n, k, mask, gt_mask, valid, focal, ws, cost_ce, cost_dice)
        cost = w_ce * cost_ce + w_dice * cost_dice.mean()
        cols = torch.empty((b, k), dtype=torch.int32, device=dev)
        nat.lsap_maximize_wrapper(b, k, -cost, cols)
        sums = torch.empty((b, k, 4), dtype=torch.float64, device=dev)
        terms = torch.empty(2, dtype=torch.float32, device=dev)
        nat.sup_mask_loss_fwd_wrapper(b, n, k, mask, gt_mask, valid, cols, focal, ws, sums, terms)
        ctx.save_for_backward(mask, gt_mask, valid, cols, sums)
        ctx.focal, ctx.w_ce, ctx.w_dice = focal, w_ce, w_dice
        ctx.mark_non_differentiable(terms, cols)
        return w_ce * terms[0] + w_dice * terms[1], terms, cols

    @staticmethod
    def backward(ctx, g_loss, _g_terms=None, _g_cols=None):
        from .. import pointnet2_cuda as nat
        mask, gt_mask, valid, cols, sums = ctx.saved_tensors
        b, n, k = mask.shape
        grad = torch.empty_like(mask)
        nat.sup_mask_loss_bwd_wrapper(b, n, k, mask, gt_mask, valid, cols, ctx.focal, sums, ctx.w_ce, ctx.w_dice,
                                      g_loss.float().reshape(1).contiguous(), grad)
        return grad, None, None, None, None, None


class PendingLossDict:
    """The monitored scalars on their way to the host (one non-blocking copy); ``resolve()`` gives the reference's loss_dict."""
    KEYS = ('cross_entropy', 'dice', 'sum')

    def __init__(self, terms):
        from ..utils.streams import HostScalars
        self._scalars = HostScalars(torch.stack([terms[k].detach().reshape(()) for k in self.KEYS]))
        self._dict = None

    def resolve(self):
        if self._dict is None:
            self._dict = dict(zip(self.KEYS, self._scalars.get()))
        return self._dict


class SupervisedMaskLoss(nn.Module):
    """Reference: :148-182; returns ``(loss, loss_dict)`` with keys cross_entropy, dice, sum."""

    def __init__(self, ce_loss, dice_loss, weights=[2.0, 0.1]):
        super().__init__()
        self.ce_loss = ce_loss
        self.dice_loss = dice_loss
        self.w_ce, self.w_dice = weights

    def kernels_apply(self, mask, gt_mask, valid=None):
        """Whether forward takes the kernel path for these inputs."""
        from .. import pointnet2_cuda as nat
        tensors = [mask, gt_mask] + ([] if valid is None else [valid])
        return (KERNELS and type(self.ce_loss) in (CrossEntropyLoss, FocalLoss) and type(self.dice_loss) is DiceLoss
                and mask.dim() == 3 and mask.shape == gt_mask.shape and 1 <= mask.shape[-1] <= nat.SUP_LOSS_MAX_K
                and mask.shape[0] >= 1 and mask.shape[1] >= 1 and (valid is None or valid.shape == mask.shape[:2])
                and (self.ce_loss.focal is None or self.ce_loss.focal[1] >= 1)
                and all(t.is_cuda and t.dtype is torch.float32 and t.is_contiguous() for t in tensors))

    def matched_labels(self, mask, gt_mask, valid=None):
        """The GT masks reordered to the predicted slots (what the loss terms are taken against), on the tensor path."""
        cost_ce, cost_dice = match_cost_tables(self.ce_loss, self.dice_loss, mask, gt_mask, valid)
        return permute_labels(gt_mask, _columns_by_cost(self.w_ce * cost_ce + self.w_dice * cost_dice.mean()))

    def forward(self, mask, gt_mask, valid=None, sync=True):
        """mask, gt_mask (B, N, K), valid (B, N) or None.  sync=False: loss_dict is a PendingLossDict (no host round trip
        here; ``resolve()`` waits for one small copy)."""
        if self.kernels_apply(mask, gt_mask, valid):
            loss, terms, _ = _FusedMaskLoss.apply(mask, gt_mask.detach(), valid, self.ce_loss.focal, float(self.w_ce),
                                                  float(self.w_dice))
            l_ce, l_dice = terms[0], terms[1]
        else:
            gt_perm = self.matched_labels(mask, gt_mask, valid)
            l_ce = self.ce_loss(mask, gt_perm, valid)
            l_dice = self.dice_loss(mask, gt_perm, valid)
            loss = self.w_ce * l_ce + self.w_dice * l_dice
        pending = PendingLossDict({'cross_entropy': l_ce, 'dice': l_dice, 'sum': loss})
        return loss, (pending.resolve() if sync else pending)
