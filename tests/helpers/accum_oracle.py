"""CPU oracle of one gradient-accumulation window (Lightning 1.3 ``accumulate_grad_batches = K``), composed from oracle.ref_cpu
only: ``(loss / K).backward()`` per micro-batch WITHOUT clearing ``.grad`` in between (autograd sums), then ONE NovoGrad step.
An incomplete window (fewer than K micro-batches: the end of an epoch) keeps the 1/K, as Lightning does.  BatchNorm runs on each
micro-batch's own statistics, like every training forward of the oracle."""
from typing import List, Sequence, Tuple

import torch

from oracle import ref_cpu as R


def train_window(model: "R.OracleModel", opt_state: "R.NovogradState", micro_batches: Sequence[tuple], K: int, lr: float,
                 wd: float = 1e-3) -> Tuple[List[float], List[torch.Tensor]]:
    """micro_batches: [(inputs, targets, pct, target_sizes), ...], at most K of them.  Returns ([loss per micro-batch], the
    accumulated gradients the optimiser stepped on, in parameter order)."""
    if not 1 <= len(micro_batches) <= K:
        raise ValueError("a window of K = %d holds 1..K micro-batches, got %d" % (K, len(micro_batches)))
    model.training = True
    model.requires_grad_(True)
    params = model.parameters()
    for p in params:
        p.grad = None
    losses = []
    for inputs, targets, pct, target_sizes in micro_batches:
        lp = model.forward(inputs, pct)
        loss = R.training_loss(lp, targets, pct, target_sizes, blank=model.n_class - 1)
        (loss if K == 1 else loss / K).backward()          # K = 1: R.train_step's own graph, bit for bit
        losses.append(float(loss.detach()))
    grads = [p.grad.detach().clone() for p in params]
    R.novograd_step([p.data for p in params], [g.clone() for g in grads], opt_state, lr, 0.8, 0.5, 1e-8, wd)
    return losses, grads
