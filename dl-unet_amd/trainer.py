"""Drop-in for the reference's trainer.py: `from trainer import training`, same signature
(trainer.py:15) and epoch bookkeeping; the step body runs on the HIP path:

    forward            unet(images)                        -> libunet_hip unet_forward
    loss (L1)          BCEWithLogitsLoss(weight=class map)  -> unet_bce_step (target from labels, fwd + grad in one pass)
    backward           loss.backward()                     -> unet_backward_stage x6 (+ RCCL all-reduce if DP)
    update (L3)        SGD(lr=1e-4, momentum=0.99)          -> unet_sgd_momentum
    (optimizer='adam' | 'adamw')  Adam / AdamW                   -> unet_adam_step
    (clip_grad_norm=max_norm)     clip_grad_norm_                -> unet_grad_sumsq, unet_grad_norm_finish (+ unet_grads_scale for SGD)
    prediction (L2)    preds.argmax(dim=1) + IoU/PE        -> unet_eval_masks (fused crop+argmax+counts)
    weight map (N3)    class_balance(labels)               -> unet_class_balance
    (loss_weights='border') weighted_map(labels)                -> unet_weighted_map
    (loss='softmax_ce')     the paper's eq. 1 for K classes       -> unet_softmax_ce_step, unet_eval_confusion
    (loss='dice' | 'ce_dice') soft Dice, alone or added to eq. 1  -> unet_dice_step

Reference behaviours kept on purpose: Q3 the dataset-name comparisons are IDENTITY tests
against string literals in the reference (trainer.py:18-27,68,110): a name arriving from argv never
passes them, a caller's literal 'ISBI2012' does (identifier-like constants are interned) and arms
the stop goal, and 'DIC-C2DH-HeLa' / 'PhC-C2DH-U373' never do (not interned), so class_balance is
always used (pinned by tests/golden/trainer_golden.json, made by running the reference);
Q4 the [B,H,W] weight map is right-aligned against [B,2,H,W] (works for B in {1,2}, raises
otherwise); Q5 only the first sample's metrics are kept per epoch.
"""
import os
import sys
from time import time

import numpy as np
import torch

from functions import class_balance, metrics_from_confusion, metrics_from_counts, weighted_map
import optim as hip_optim


def maybe_mkdir_p(path):
    os.makedirs(path, exist_ok=True)


_PROGRESS_FILES = (('train_iou', 'train_eval_iou.out'), ('train_pe', 'train_eval_pe.out'), ('val_iou', 'val_eval_iou.out'),
                   ('val_pe', 'val_eval_pe.out'), ('loss', 'loss.out'), ('loss_val', 'loss_val.out'))


def _f6(v):
    return "{:.6f}".format(v)


def _report(rows):
    """The epoch summary on stdout, label column 27 wide as in the reference's prints (trainer.py:150-160)."""
    for label, text in rows:
        print('%-27s %s' % (label, text))
    print(' ')


def _save_weights(unet, fold_dir, tag, before=None):
    """models/unet_weight_save_<tag>.pth + the reference's two announcement lines (trainer.py:143-147 and its siblings)."""
    path = os.path.join(fold_dir, 'models', 'unet_weight_save_{}.pth'.format(tag))
    torch.save(unet.state_dict(), path)
    if before is not None:
        print(before)
    print('Model has been saved:')
    print(path)


def _goal_for(DATASET):
    """(when_to_stop, goal) exactly as the reference's `DATASET is '<literal>'` chain decides it
    (trainer.py:18-27).  Which object a caller can hold: CPython interns identifier-like string
    constants, so any module's literal 'ISBI2012' IS the reference's constant (sys.intern returns
    that same object); 'DIC-C2DH-HeLa' and 'PhC-C2DH-U373' contain '-', are not interned, and the
    reference's private constant objects can be reached by no caller: those branches never fire.
    The ISBI2012 goal (a pixel-error value, 0.0611) is tested against the validation IoU, as there."""
    if DATASET is sys.intern('ISBI2012'):
        return 1, 0.0611
    return None, None


_LOSS_WEIGHTS = {'class_balance': class_balance, 'border': weighted_map, 'none': None}
_LOSSES = ('bce', 'softmax_ce', 'dice', 'ce_dice')
_DICE_DEFAULTS = {'dice': dict(ce_weight=0.0, dice_weight=1.0), 'ce_dice': dict(ce_weight=1.0, dice_weight=1.0)}
_DICE_OPTIONS = ('smooth', 'batch', 'include_background', 'ce_weight', 'dice_weight')


def dice_step_options(loss, dice_options=None):
    """The keyword arguments optim.dice_step gets for loss = 'dice' | 'ce_dice': the loss's default weights ((0, 1) and (1, 1))
    overridden by `dice_options`; None for the other losses.  Raises ValueError for an unknown key, and for dice_options
    given with a loss that does not use them."""
    if loss not in _DICE_DEFAULTS:
        if dice_options:
            raise ValueError("dice_options are for loss='dice' and loss='ce_dice', got loss=%r" % (loss,))
        return None
    opts = dict(_DICE_DEFAULTS[loss])
    if dice_options is not None:
        unknown = sorted(set(dice_options) - set(_DICE_OPTIONS))
        if unknown:
            raise ValueError("unknown dice_options %s (known: %s)" % (unknown, list(_DICE_OPTIONS)))
        opts.update(dice_options)
    if loss == 'dice' and float(opts['ce_weight']) != 0.0:
        raise ValueError("loss='dice' has no cross-entropy term (ce_weight=%r); loss='ce_dice' is the sum" % (opts['ce_weight'],))
    return opts


def _step_loss(unet, images, labels, device, train, weight_fn=class_balance, loss_kind='bce', validate=False, dice_kw=None):
    preds = unet(images.to(device))
    labels = labels.to(device)                                  # everything below stays on the device
    pad = int((preds.shape[-1] - labels.shape[-1]) / 2)
    preds = preds[:, :, pad:labels.shape[-1] + pad, pad:labels.shape[-1] + pad]
    weight_maps = weight_fn(labels.squeeze(1)) if weight_fn is not None else None   # [B,H,W] (trainer.py:72 / :70)
    if dice_kw is not None:
        # soft Dice (+ eq. 1): the weight map, if any, multiplies the cross-entropy term only
        loss, _ = hip_optim.dice_step(preds, labels, weight=weight_maps, want_mask=False, validate=validate, **dice_kw)
    elif loss_kind == 'softmax_ce':
        # eq. 1: the weight map multiplies each pixel's cross-entropy (per pixel, not Q4's class-axis alignment)
        loss, _ = hip_optim.softmax_ce_step(preds, labels, weight=weight_maps, want_mask=False, validate=validate)
    else:
        # the one-hot target [1-y, y] (trainer.py:63-66) is formed inside the kernel from the integer labels
        loss, _ = hip_optim.bce_argmax_step(preds, labels, weight=weight_maps, want_mask=False)
    return preds, loss, labels


def _first_sample_metrics(preds, labels):
    """argmax + IoU / pixel error of the batch in one device pass; only sample 0 is kept (quirk Q5).  Binary heads count
    with unet_eval_masks; K-class heads with the confusion counts (IoU = mean over the foreground classes)."""
    if preds.shape[1] != 2:
        _, conf = hip_optim.crop_argmax_confusion(preds.detach(), labels)
        return metrics_from_confusion(conf[0].cpu().numpy())
    _, stats = hip_optim.crop_argmax_metrics(preds.detach(), labels)
    inter, union, diff = [int(v) for v in stats[0].tolist()]
    return metrics_from_counts(inter, union, diff, labels.shape[-1] * labels.shape[-2])


def check_loss_options(n_classes, loss, loss_weights):
    """Raises ValueError for a combination training() cannot run, before any device work."""
    if loss not in _LOSSES:
        raise ValueError("loss must be one of %s, got %r" % (list(_LOSSES), loss))
    if loss_weights not in _LOSS_WEIGHTS:
        raise ValueError("loss_weights must be one of %s, got %r" % (sorted(_LOSS_WEIGHTS), loss_weights))
    if loss == 'dice' and loss_weights != 'none':
        raise ValueError("loss='dice' has no cross-entropy term for loss_weights=%r to weight; it takes loss_weights='none' "
                         "(loss='ce_dice' weights its cross-entropy term)" % (loss_weights,))
    if n_classes != 2:
        if loss == 'bce':
            raise ValueError("loss='bce' is the reference's two-class loss; a %d-class net trains with loss='softmax_ce'" % n_classes)
        if loss_weights != 'none':
            raise ValueError("loss_weights=%r is defined for {0,1} labels only; a %d-class net takes loss_weights='none'"
                             % (loss_weights, n_classes))


_OPTIMIZERS = {'sgd': (hip_optim.SGD, ('lr', 'momentum'), dict(lr=0.0001, momentum=0.99)),
               'adam': (hip_optim.Adam, ('lr', 'betas', 'eps', 'weight_decay'), dict(lr=0.0001)),
               'adamw': (hip_optim.AdamW, ('lr', 'betas', 'eps', 'weight_decay'), dict(lr=0.0001))}


def check_optimizer_options(optimizer='sgd', optimizer_options=None, clip_grad_norm=None):
    """The keyword arguments the optimiser of training(optimizer=...) is built with: lr = 1e-4 for all three (momentum = 0.99
    for 'sgd'; the other defaults are optim.Adam's and optim.AdamW's) overridden by `optimizer_options`.  Raises ValueError,
    before any device work, for an unknown optimizer, an unknown key (known: lr, momentum for 'sgd'; lr, betas, eps,
    weight_decay for 'adam' and 'adamw'), a value the optimiser does not take, and a clip_grad_norm that is neither None nor a
    positive number."""
    if optimizer not in _OPTIMIZERS:
        raise ValueError("optimizer must be one of %s, got %r" % (sorted(_OPTIMIZERS), optimizer))
    _, known, defaults = _OPTIMIZERS[optimizer]
    opts = dict(defaults)
    if optimizer_options is not None:
        unknown = sorted(set(optimizer_options) - set(known))
        if unknown:
            raise ValueError("unknown optimizer_options %s for optimizer=%r (known: %s)" % (unknown, optimizer, list(known)))
        opts.update(optimizer_options)
    if optimizer == 'sgd':
        for k in ('lr', 'momentum'):
            if not (float(opts[k]) >= 0.0 and np.isfinite(float(opts[k]))):
                raise ValueError("optimizer_options: %s must be >= 0, got %r" % (k, opts[k]))
    else:
        hip_optim.check_adam_options(**opts)
    if clip_grad_norm is not None and not (isinstance(clip_grad_norm, (int, float)) and float(clip_grad_norm) > 0.0
                                           and np.isfinite(float(clip_grad_norm))):
        raise ValueError("clip_grad_norm must be None or a positive number, got %r" % (clip_grad_norm,))
    return opts


def training(unet, train_loader, val_loader, epochs, batch_size, device, fold_dir, DATASET, *, resume_from=None,
             save_optimizer=False, loss_weights='class_balance', loss='bce', dice_options=None, optimizer='sgd',
             optimizer_options=None, clip_grad_norm=None):
    """Reference signature (trainer.py:15) plus keyword-only extensions, all off by default so that the files
    written are exactly the reference's: resume_from = a checkpoint made by checkpoint.py (weights + SGD momentum +
    scheduler + epoch), save_optimizer = also write models/checkpoint_latest.pth every epoch (both SURVEY N4);
    loss_weights = 'border' weights the training and the validation loss with weighted_map (the paper's border
    map, what the reference's HeLa branch asks for at trainer.py:68-70,110-112) instead of class_balance.
    loss = 'softmax_ce' trains with the paper's eq. 1 (optim.softmax_ce_step, a pixel-wise soft-max over the classes with a
    weighted cross-entropy) instead of the reference's per-channel BCE ('bce', the default).  A net with n_classes = K > 2
    needs loss='softmax_ce' and loss_weights='none' (uniform; class_balance and 'border' are defined for {0,1} labels), and
    its IoU / PE series come from the confusion counts (mean IoU over the foreground classes; first sample, Q5).  With K = 2,
    both losses take all three loss_weights: loss='bce' with loss_weights='none' is the reference's BCE without a weight map
    (uniform), 'softmax_ce' with 'class_balance' / 'border' weights each pixel's cross-entropy by the map.  Labels are validated (an error if any is outside [0, K)) on the first
    training step of every epoch only: the check reads a count back to the host, and a sync on every step would add host gap
    to every step; labels outside [0, K) in the other steps add no loss and no gradient.
    loss = 'dice' trains with the soft Dice loss over the soft-max (optim.dice_step), loss = 'ce_dice' with its sum with eq. 1
    (nnU-Net's default); both are valid for every K >= 2.  'ce_dice' follows 'softmax_ce' for loss_weights (all three at K = 2,
    weighting the cross-entropy term; 'none' at K > 2); 'dice' has no term to weight and takes loss_weights='none' only.
    dice_options = a dict of smooth, batch, include_background, ce_weight, dice_weight (dice_step's; unknown keys raise); the
    weights default to (0, 1) for 'dice' and (1, 1) for 'ce_dice'.  Under dp.DataParallel every rank forms the Dice
    coefficients on its own shard of the batch, then the gradients are averaged: batch=True means the rank's batch, not the
    global one.
    optimizer = 'sgd' (the reference's SGD with momentum 0.99, the default), 'adam' or 'adamw' (optim.Adam / optim.AdamW, one
    unet_adam_step launch per step); optimizer_options = a dict of lr, momentum ('sgd') or lr, betas, eps, weight_decay ('adam',
    'adamw'); unknown keys raise.  lr defaults to 1e-4 for all three: a choice, not a tuned value; the scheduler is the same.
    clip_grad_norm = None, or max_norm > 0: the global 2-norm of the gradients is formed on the device after backward
    (optim.clip_grad_norm_, no host sync) and the gradients are scaled by min(1, max_norm / (norm + 1e-6)): inside the Adam
    pass for 'adam' / 'adamw', in place before the update for 'sgd'.  Under dp.DataParallel the norm is that of the reduced
    gradients, the same bits on every rank.  resume_from a checkpoint written with another kind of optimiser raises
    ValueError (checkpoint.load_checkpoint); with save_optimizer the Adam state (step, exp_avg, exp_avg_sq) is saved and a
    resumed run is the interrupted one, as for SGD."""
    n_classes = getattr(unet, 'n_classes', 2)
    check_loss_options(n_classes, loss, loss_weights)
    dice_kw = dice_step_options(loss, dice_options)
    optimizer_kw = check_optimizer_options(optimizer, optimizer_options, clip_grad_norm)
    fused_clip = optimizer != 'sgd'                             # Adam takes the clipping coefficient inside its own pass
    weight_fn = _LOSS_WEIGHTS[loss_weights]
    loss_kind = loss
    when_to_stop, goal = _goal_for(DATASET)

    optimizer = _OPTIMIZERS[optimizer][0](unet.parameters(), **optimizer_kw)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode='min', factor=0.1, patience=30,
                                                           threshold=1e-3, threshold_mode='rel', eps=1e-7)
    my_patience = 0
    first_epoch = 0
    if resume_from is not None:
        import checkpoint
        extra = checkpoint.load_checkpoint(resume_from, unet, optimizer, scheduler)
        first_epoch = int(extra.get("epoch", -1)) + 1
        my_patience = int(extra.get("my_patience", 0))
        resumed_best = extra.get("loss_best_epoch")
        if extra.get("goal_armed") is False:                   # the goal had been reached (and cleared) before the interruption
            when_to_stop = None
    else:
        resumed_best = None
        extra = {}

    maybe_mkdir_p(os.path.join(fold_dir, 'progress'))
    maybe_mkdir_p(os.path.join(fold_dir, 'models'))

    loss_best_epoch = 100000.0 if resumed_best is None else float(resumed_best)
    progress = {k: None for k in ('train_iou', 'train_pe', 'val_iou', 'val_pe', 'loss', 'loss_val')}
    for k, v in (extra.get("progress") or {}).items():         # a resumed run goes on writing the interrupted run's series
        if k in progress and len(v):
            progress[k] = np.array(v, dtype=np.float64)

    epoch = first_epoch - 1
    for epoch in range(first_epoch, epochs + 1):
        print(' ')
        print('Epoch:', epoch)
        start = time()
        total_loss = 0
        total_loss_val = 0
        train_eval = None
        val_eval = None

        for step, (images, labels) in enumerate(train_loader):
            optimizer.zero_grad()
            preds, loss, labels = _step_loss(unet, images, labels, device, True, weight_fn, loss_kind, step == 0, dice_kw)
            loss.backward()
            if clip_grad_norm is None:
                optimizer.step()
            else:
                _, coef = hip_optim.clip_grad_norm_(unet.parameters(), clip_grad_norm, scale=not fused_clip)
                if fused_clip:
                    optimizer.step(grad_scale=coef)
                else:
                    optimizer.step()
            total_loss += loss.detach()
            if train_eval is None:                              # Q5: first sample of the epoch only
                train_eval = _first_sample_metrics(preds, labels)
        train_eval_epoch = np.mean(train_eval, axis=1)

        with torch.no_grad():
            for images, labels in val_loader:
                preds, loss, labels = _step_loss(unet, images, labels, device, False, weight_fn, loss_kind, dice_kw=dice_kw)
                total_loss_val += loss
                if val_eval is None:
                    val_eval = _first_sample_metrics(preds, labels)
        val_eval_epoch = np.mean(val_eval, axis=1)

        scheduler.step(total_loss_val / (len(val_loader) * batch_size))
        for param_group in optimizer.param_groups:
            l_rate = param_group['lr']

        loss_epoch = total_loss / (len(train_loader) * batch_size)
        loss_epoch_val = total_loss_val / (len(val_loader) * batch_size)

        improved = loss_epoch_val < (loss_best_epoch * (1.0 - scheduler.threshold))
        if improved:
            loss_best_epoch = loss_epoch_val
            print('New best epoch!')
            _save_weights(unet, fold_dir, 'best')
        my_patience = 0 if improved else my_patience + 1

        _report((('Current lr is:', l_rate),
                 ('Patience is:', '{}/{}'.format(my_patience, scheduler.patience)),
                 ('Mean IoU training:', _f6(train_eval_epoch[0])), ('Mean PE training:', _f6(train_eval_epoch[1])),
                 ('Mean IoU validation:', _f6(val_eval_epoch[0])), ('Mean PE validation:', _f6(val_eval_epoch[1])),
                 ('Total training loss:', _f6(loss_epoch.item())), ('Total validation loss:', _f6(loss_epoch_val.item())),
                 ('Best epoch validation loss:', _f6(float(loss_best_epoch))),
                 ('Epoch duration:', _f6(time() - start) + ' s')))

        # the six progress series, one value per epoch, rewritten whole every epoch (trainer.py:162-183)
        new = dict(train_iou=train_eval_epoch[0], train_pe=train_eval_epoch[1], val_iou=val_eval_epoch[0],
                   val_pe=val_eval_epoch[1], loss=loss_epoch.item(), loss_val=loss_epoch_val.item())
        for k, fname in _PROGRESS_FILES:
            progress[k] = np.array([new[k]]) if progress[k] is None else np.append(progress[k], [new[k]])
            np.savetxt(os.path.join(fold_dir, 'progress', fname), progress[k])

        if save_optimizer:
            import checkpoint
            # state as it is at the END of this epoch: the patience reset and the goal test below are anticipated
            armed_after = when_to_stop is not None and not (val_eval_epoch[0] > goal)
            patience_after = my_patience
            if when_to_stop is None and my_patience == scheduler.patience:
                patience_after = -1
            checkpoint.save_checkpoint(os.path.join(fold_dir, 'models', 'checkpoint_latest.pth'), unet, optimizer, scheduler,
                                       epoch=epoch, my_patience=patience_after, loss_best_epoch=float(loss_best_epoch),
                                       goal_armed=armed_after, progress={k: [float(x) for x in v] for k, v in progress.items()})

        if when_to_stop is not None:
            # goal armed (trainer.py:185-214): the periodic checkpoint and the LR-floor stop are skipped this epoch
            if val_eval_epoch[0] > goal:
                _save_weights(unet, fold_dir, DATASET, before='The goal was reached in epoch {}!'.format(epoch))
                when_to_stop = None
            continue

        if epoch % 25 == 0:
            _save_weights(unet, fold_dir, 'latest')

        lr_floor = 10 * scheduler.eps
        out_of_patience = my_patience == scheduler.patience
        if l_rate < lr_floor and out_of_patience:
            for line in (f'LR dropped below {lr_floor}!', 'Stopping training', ' '):
                print(line)
            _save_weights(unet, fold_dir, 'latest')
            break
        if out_of_patience:
            my_patience = -1

    print('Training is finished as epoch {} has been reached'.format(epoch))
    print(' ')
