"""The reference's classification training loop (classify/train.py:154-160, 176-290) on the yolov5_amd seams, in its order and with its defaults.

MI355X mapping: the train-mode forward and the backward are the TrainEngine plan (the Classify head's pool + Dropout + Linear and its backward:
csrc/classify_train.h), the loss is y5_classify_post with y5_classify_ce_bwd as its gradient, the optimizer block is HipSGD.step_fused for SGD
(unscale + clip + step + EMA in three launches) and train_loop.host_amp_step for the torch optimizers (Adam is the reference's default here);
fused_optimizer=True puts Adam / AdamW / RMSProp on the same device path (torch_utils.HipAdam / HipAdamW / HipRMSprop: four launches, the step count
and the overflow flag stay on the device).  Validation is classify_val.run on the EMA model.

Not here: warm-up and gradient accumulation (the reference's classification loop has neither), classify_albumentations(augment=True) (without
albumentations the reference trains on torch_transforms as well: dataloaders.ClassificationLoader), image folders, torchvision models, plots,
loggers, and the DDP launch plumbing (the engine tells a HipDDP sink about the Linear's gradients like any other; a multi-rank run is not built).
"""
from __future__ import annotations

from pathlib import Path

import torch

from . import classify_val
from .torch_utils import ModelEMA, smart_optimizer, smartCrossEntropyLoss
from .train_loop import LossScaler, host_amp_step, lr_lambda


def train(model, trainloader, testloader=None, epochs=10, optimizer_name="Adam", lr0=0.001, decay=5e-5, label_smoothing=0.1, dropout=None, amp=True,
          ema=True, max_norm=10.0, pretrained=True, save_dir=None, on_batch_end=None, fused_optimizer=False):
    """Runs `epochs` epochs over `trainloader` (re-iterable of (images (b, 3, s, s) float, labels (b)) batches on the model's device).  amp: fp16
    images select the fp16 plan and the loss is scaled (GradScaler's policy: train_loop.LossScaler); amp=False feeds fp32 images to the fp32 plan.
    testloader: validated once per epoch with the EMA model (the live model without an EMA), fitness = top-1 accuracy.  save_dir: last.pt / best.pt
    as classify/train.py:271-289 writes them (the fp16 copy of the EMA as "model", no optimizer state).  fused_optimizer: smart_optimizer(fused=True).
    Returns dict(model, ema, optimizer, scheduler, scaler, losses (iterations,), tloss / vloss / top1 / top5 / lr per epoch, best_fitness)."""
    for m in model.modules():                                                       # :154-158
        if not pretrained and hasattr(m, "reset_parameters"):
            m.reset_parameters()
        if isinstance(m, torch.nn.Dropout) and dropout is not None:
            m.p = dropout
    for p in model.parameters():
        p.requires_grad = True                                                      # :159-160
    optimizer = smart_optimizer(model, optimizer_name, lr0, momentum=0.9, decay=decay, fused=fused_optimizer)   # :176
    scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=lr_lambda(epochs, 0.01))   # :179-186 (linear, lrf = 0.01)
    ema_obj = ModelEMA(model) if ema else None                                      # :191
    criterion = smartCrossEntropyLoss(label_smoothing=label_smoothing)              # :199
    best_fitness = 0.0
    scaler = LossScaler(enabled=amp)                                                # :202
    fused = hasattr(optimizer, "step_fused")
    hist = {"losses": [], "tloss": [], "vloss": [], "top1": [], "top5": [], "lr": []}
    if save_dir is not None:
        save_dir = Path(save_dir)
        save_dir.mkdir(parents=True, exist_ok=True)
    ni = 0
    for epoch in range(epochs):                                                     # :211
        tloss, vloss, fitness, top1, top5 = None, 0.0, 0.0, 0.0, 0.0
        model.train()
        for i, (images, labels) in enumerate(trainloader):
            x = images.half() if amp else images.float()
            loss = criterion(model(x), labels)                                      # :223-224
            (loss * scaler.scale).backward()                                        # :227
            if fused:                                                               # :230-236
                scaler.record(optimizer.step_fused(inv_scale=1.0 / scaler.scale, max_norm=max_norm, ema=ema_obj, model=model))
            else:
                host_amp_step(optimizer, model.parameters(), scaler, max_norm)
                if ema_obj is not None:
                    ema_obj.update(model)
            scaler.update()
            optimizer.zero_grad()
            ld = loss.detach().float()
            tloss = ld if tloss is None else (tloss * i + ld) / (i + 1)             # :240 (kept on the device: one read per epoch)
            hist["losses"].append(ld)
            if on_batch_end is not None:
                on_batch_end(ni, ld, optimizer)
            ni += 1
        scheduler.step()                                                            # :252
        if testloader is not None:                                                  # :245-249
            top1, top5, vloss = classify_val.run(ema_obj.ema if ema_obj is not None else model, testloader, criterion=criterion)
            fitness = top1
        best_fitness = max(best_fitness, fitness)                                   # :257
        hist["tloss"].append(float(tloss) if tloss is not None else 0.0)
        hist["vloss"].append(float(vloss))
        hist["top1"].append(float(top1))
        hist["top5"].append(float(top5))
        hist["lr"].append(optimizer.param_groups[0]["lr"])                          # :265
        if save_dir is not None:                                                    # :270-288
            from .checkpoint import save_checkpoint

            src = ema_obj.ema if ema_obj is not None else model
            save_checkpoint(save_dir / "last.pt", src, ema=None, optimizer=None, epoch=epoch, best_fitness=best_fitness)
            if best_fitness == fitness:
                save_checkpoint(save_dir / "best.pt", src, ema=None, optimizer=None, epoch=epoch, best_fitness=best_fitness)
    scaler.update(block=True)
    hist["losses"] = torch.stack(hist["losses"]).cpu() if hist["losses"] else torch.zeros(0)
    return dict(model=model, ema=ema_obj, optimizer=optimizer, scheduler=scheduler, scaler=scaler, best_fitness=best_fitness, **hist)
