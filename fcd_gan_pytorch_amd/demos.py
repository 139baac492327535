"""Runnable restatements of the reference's three demo scripts on the HIP path
(Demo_USSS.py / Demo_RSSS.py / Demo_WSSS.py are ``if __name__ == '__main__'`` blocks with
hard-coded paths; these are the same phases as functions with the knobs as arguments).

Only the orchestration lives here: tile feeding (``tiles``), the step bodies (``steps``),
the LR schedule, on-device metrics (``metrics``), inference + centre write-back.  Logging
to TensorBoard, ``Para*.txt`` dumps and ETA printing are out of scope.
"""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import Loss, Module, datasets, dp, metrics, optim, steps, tiles
from . import transforms as _transforms


class _Epoch:
    """One pass over a dataset, data-parallel aware: rank-strided batches off a shared per-epoch permutation
    (``dp.RankStridedBatches``), pinned-memory prefetch, and per-batch sample weights that leave out the padded
    duplicates of a ragged last batch.  Iterating yields ``(batch, n_real, weight)`` with
    ``weight = n_real / len(dataset)`` so that ``sum(weight * batch_mean)`` over all ranks is the epoch mean the
    reference logs (Demo_RSSS.py:334-343)."""

    def __init__(self, ds, batch_size, seed, device, shuffle=True, wrap=None, ragged='pad'):
        self.ds, self.device, self.wrap = ds, device, wrap
        self.sampler = dp.RankStridedBatches(len(ds), batch_size, seed=seed, shuffle=shuffle, ragged=ragged)

    def __iter__(self):
        loader = DataLoader(self.ds, batch_sampler=self.sampler)
        it = self.wrap(loader) if self.wrap else loader
        for i, batch in enumerate(tiles.Prefetcher(it, self.device)):
            n = batch[0].shape[0]
            real = n - self.sampler.pads[i]
            w = _Weight(real / float(len(self.ds)))
            w.loss_scale = self.sampler.scales[i]         # != 1 only in the last batch under ragged='weighted' (pass to the step)
            yield batch, real, w


class _Weight(float):
    """The batch's epoch weight (a float) that also carries the loss scale of the step (``dp`` ragged='weighted')."""
    loss_scale = 1.0


def _real_mask(like, real):
    """(N,1,1,1) bool: True for the first ``real`` samples of the batch (padded duplicates come last)."""
    m = torch.zeros((like.shape[0], 1, 1, 1), dtype=torch.bool, device=like.device)
    m[:real] = True
    return m


def _epoch_mean(total):
    """Sum of the ranks' weighted partial sums (each rank saw its share of the samples)."""
    return dp.sum_counts(total.double())


def _save(net, path):
    """``torch.save(net.state_dict(), path)`` on rank 0 (Demo_RSSS.py:507-514, Demo_USSS.py:477-481)."""
    if path and dp.world_info()[0] == 0:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        torch.save(net.state_dict(), path)


def _tile_stats(scene_x, scene_y, patch_size, stats_txt=None):
    """Dataset_meanstd over the NON-overlapped tiling of the scene pair (Demo_USSS.py:88-95): per-tile means weighted
    by valid-pixel counts, cached in the reference's two text files when ``stats_txt=(path_x, path_y)``."""
    ds = tiles.PairTileDataset(scene_x, scene_y, None, patch_size, (0, 0))
    if stats_txt:
        return tuple(np.asarray(v, np.float64) for v in tiles.dataset_meanstd(stats_txt[0], stats_txt[1], ds))
    mx, my = tiles.dataset_mean(ds)
    sx, sy = tiles.dataset_std(ds, mx, my)
    return tuple(v.double().numpy() for v in (mx, sx, my, sy))


def _tile_ranges(scene_x, scene_y, patch_size, stats_txt=None):
    """Dataset_maxmin over the NON-overlapped tiling of the scene pair (Demo_RSSS.py:91-96): two lists of [min, max] per band,
    cached in the reference's two text files when ``stats_txt=(path_x, path_y)``."""
    ds = tiles.PairTileDataset(scene_x, scene_y, None, patch_size, (0, 0))
    if stats_txt:
        return tiles.dataset_maxmin(stats_txt[0], stats_txt[1], ds)
    return tiles._fold_maxmin(ds)


def demo_usss(scene_x, scene_y, ref=None, device='cuda', patch_size=(220, 220), overlap_padding=(10, 10),
              epochs_g=50, epochs_s=50, epochs_joint=100, batch_size=10, learning_rate=2e-4,
              perception_weight=0.4, l1_weight=0.65, ssim_weight=0, perception_perBand=True,
              prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1), seed=0, out_density=None, out_color=None,
              log=None, allow_seeded=False, stats_txt=None, save_s=None, save_g=None, ragged='pad', resident_inference=False,
              resident_training=False, enhance='normalize', scale_range=(-1, 1), transforms=None):
    """Demo_USSS.py:29-501: G pre-train -> S pre-train -> joint training -> inference with centre write-back, with the
    reference's LR schedules (Demo_USSS.py:133,201,298-299) and per-tile dataset statistics (:88-95).
    ``scene_x/scene_y/ref``: (bands,H,W) arrays or TIFF paths; ``save_s`` / ``save_g``: ``.pkl`` paths
    (Demo_USSS.py:477-481).  ``batch_size`` is per rank under data parallelism.  ``resident_inference=True`` runs the final
    inference with the scene pair and the maps resident on the device (``infer_scene_resident``: same maps and scores).
    ``resident_training=True`` uploads ONE ``tiles.ResidentScene`` that serves the statistics (``scene.statistics`` /
    ``tiles.scene_meanstd`` when ``stats_txt`` is given: exact moments, equal to the host's to about seven digits), all three
    training phases (``ResidentSceneSet.epoch``: same batches, tiles bit-identical for the same statistics), the joint phase's
    accuracy (counted over each tile's owned centre, ``Evaluator.add_tiles`` on resident rectangles -- with overlapped tiles
    the host route counts the context ring too) and the final inference.
    ``enhance``: 'normalize' (NORMALIZE with the tile statistics), or the reference's alternative pre-processing 'scale' /
    'scale_norm' (``transforms.SCALE`` / ``SCALE_NORM`` onto ``scale_range``) with the per-band ranges of
    ``tiles.dataset_maxmin`` (host route) or ``scene.maxmin()`` (resident route), cached through ``stats_txt`` when given; both
    training routes and both inference routes use the same enhancer.  ``transforms``: a ``transforms.RANDOM_ERASER`` /
    ``RANDOM_ERASER_MULTI_REGION`` for the TRAINING tiles only (drawn per tile on the host route, per epoch plan on the resident
    one); inference never erases.
    Returns dict(netS, netG, density (1,H,W) float32, color (1,H,W), evaluator, history, vgg_pretrained)."""
    dev = torch.device(device)
    if isinstance(scene_x, str):
        scene_x = tiles.read_tiff(scene_x)
    if isinstance(scene_y, str):
        scene_y = tiles.read_tiff(scene_y)
    if isinstance(ref, str):
        ref = tiles.read_tiff(ref)
    if enhance not in ('normalize', 'scale', 'scale_norm'):
        raise ValueError("enhance: 'normalize', 'scale' or 'scale_norm', got %r" % (enhance,))
    scene, stats, enh = None, None, None
    if resident_training:
        scene = tiles.ResidentScene(scene_x, scene_y, ref, patch_size, overlap_padding, device=dev)
        if enhance == 'normalize':
            stats = tiles.scene_meanstd(stats_txt[0], stats_txt[1], scene) if stats_txt else scene.statistics()
            stats = tuple(np.asarray(v, np.float64) for v in stats)
            scene.set_stats(stats)
        else:
            r1, r2 = tiles.scene_maxmin(stats_txt[0], stats_txt[1], scene) if stats_txt else scene.maxmin()
            enh = _transforms.enhancer(enhance, r1, r2, scale_range)
            scene.set_enhance(enh)
        feed = tiles.ResidentSceneSet([scene], transforms=transforms)
        epoch = lambda sd: feed.epoch(batch_size, sd, ragged=ragged)
    else:
        if enhance == 'normalize':
            stats = _tile_stats(scene_x, scene_y, patch_size, stats_txt)
        else:
            r1, r2 = _tile_ranges(scene_x, scene_y, patch_size, stats_txt)
            enh = _transforms.enhancer(enhance, r1, r2, scale_range)
        epoch = lambda sd: _Epoch(train_ds, batch_size, sd, dev, ragged=ragged)
    ds = tiles.PairTileDataset(scene_x, scene_y, ref, patch_size, overlap_padding, stats=stats, enhance=enh)
    # the erasers augment the training tiles only: inference reads ``ds``, which never has them
    train_ds = ds if transforms is None else tiles.PairTileDataset(scene_x, scene_y, ref, patch_size, overlap_padding,
                                                                   stats=stats, enhance=enh, transforms=transforms)
    nband = scene_x.shape[0]
    torch.manual_seed(seed)
    netS = Module.Segmentor(n_channels=nband, bilinear=True).to(dev)
    netG = Module.Generator(n_channels=nband).to(dev)
    crit = Loss.CNetLoss(channel=nband, perception_layer=1, perception_perBand=perception_perBand,
                         allow_seeded=allow_seeded).to(dev)
    netS.train(); netG.train()                                                    # Demo_USSS.py:116-117
    optS = optim.Adam(netS.parameters(), lr=learning_rate, betas=(0.9, 0.99))
    optG = optim.Adam(netG.parameters(), lr=learning_rate, betas=(0.9, 0.99))
    dp.sync_start((netS, netG), (optS, optG))
    hist = {'g': [], 's': [], 'joint': []}
    acc = metrics.Evaluator(2)
    kw = dict(perception_weight=perception_weight, ssim_weight=ssim_weight)

    for ep in range(epochs_g):                                                   # Demo_USSS.py:126-189
        optim.adjust_learning_rate(optG, ep, lr_start=1e-5, lr_max=3e-4, lr_warm_up_epoch=10, lr_sustain_epochs=10)
        tot = torch.zeros((), device=dev)
        for (x, y, item, r), real, w in epoch(seed * 1000 + ep):
            out = steps.usss_g_pretrain_step(netG, crit, optG, x, y, **kw, loss_scale=w.loss_scale)
            tot += out['loss'].detach() * w
        hist['g'].append(float(_epoch_mean(tot)))
        if log:
            log('G pre-train epoch %d loss %.4f' % (ep + 1, hist['g'][-1]))
    for ep in range(epochs_s):                                                   # Demo_USSS.py:194-286
        optim.adjust_learning_rate(optS, ep, lr_start=1e-5, lr_max=3e-4, lr_warm_up_epoch=10, lr_sustain_epochs=10)
        tot = torch.zeros((), device=dev)
        for (x, y, item, r), real, w in epoch(seed * 1000 + 1000 + ep):
            out = steps.usss_s_pretrain_step(netS, netG, crit, optS, x, y, l1_weight=l1_weight, **kw, loss_scale=w.loss_scale)
            tot += out['net_loss'].detach() * w
        hist['s'].append(float(_epoch_mean(tot)))
        if log:
            log('S pre-train epoch %d loss %.4f' % (ep + 1, hist['s'][-1]))
    for ep in range(epochs_joint):                                               # Demo_USSS.py:291-400
        optim.adjust_learning_rate(optS, ep, lr_start=1e-5, lr_max=1e-4)
        optim.adjust_learning_rate(optG, ep, lr_start=1e-5, lr_max=1e-4)
        tot = torch.zeros((), device=dev)
        acc.reset()
        for (x, y, item, r), real, w in epoch(seed * 1000 + 2000 + ep):
            out = steps.usss_joint_step(netS, netG, crit, optS, optG, x, y, l1_weight=l1_weight, **kw, loss_scale=w.loss_scale)
            tot += out['net_loss'].detach() * w
            if ref is not None and resident_training:
                if w.rects is not None:
                    acc.add_tiles(r, out['cmap'].detach(), w.rects, prob_thresh, gt_map, pre_map)
            elif ref is not None:
                acc.add_batch_map(r, metrics.threshold_map(out['cmap'].detach(), prob_thresh), gt_map, pre_map,
                                  valid=_real_mask(r, real).expand_as(r))
        hist['joint'].append(float(_epoch_mean(tot)))
        if log:
            log('joint epoch %d loss %.4f' % (ep + 1, hist['joint'][-1]))

    dp.sync_buffers((netS, netG))            # one set of BatchNorm statistics for the stitched map AND the checkpoint
    if resident_inference:
        if scene is None:
            scene = tiles.ResidentScene(scene_x, scene_y, ref, patch_size, overlap_padding, stats=stats, device=dev, enhance=enh)
        res = infer_scene_resident(netS, scene, dev, batch_size=batch_size, prob_thresh=prob_thresh, gt_map=gt_map,
                                   pre_map=pre_map)
    else:
        res = infer_scene(netS, ds, dev, batch_size=batch_size, prob_thresh=prob_thresh, gt_map=gt_map, pre_map=pre_map)
    if out_density and dp.world_info()[0] == 0:
        tiles.write_tiff(out_density, res['density'])
    if out_color and dp.world_info()[0] == 0:
        tiles.write_tiff(out_color, res['color'])
    _save(netS, save_s)
    _save(netG, save_g)
    res.update(netS=netS, netG=netG, history=hist, train_evaluator=acc, vgg_pretrained=crit.loss_perception.pretrained)
    return res


@torch.no_grad()
def infer_scene(netS, ds, device, batch_size=10, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1), eval_mode=True):
    """Inference over every tile of a PairTileDataset with centre write-back
    (Demo_USSS.py:404-470, Demo_RSSS.py:451-491): density map (float32), TP/FP/FN colour codes
    and the evaluator over the owned centres.  ``eval_mode=False`` keeps train() statistics
    like Demo_WSSS.py:389-391.  Under data parallelism the tiles are sharded rank-strided; every
    centre is owned by exactly one tile, so the stitched maps are the SUM over ranks; in eval mode rank 0's BatchNorm
    running statistics are broadcast first (``dp.sync_buffers``) so every tile is normalised alike and the map equals
    what rank 0's checkpoint reproduces."""
    dev = torch.device(device)
    if eval_mode:
        dp.sync_buffers((netS,))
    was_training = netS.training
    netS.train(not eval_mode)
    grid = ds.grid
    density = np.zeros((1, grid.ysize, grid.xsize), np.float32)
    color = np.zeros((1, grid.ysize, grid.xsize), np.float32)
    acc = metrics.Evaluator(2)
    for (x, y, item, r), real, _ in _Epoch(ds, batch_size, 0, dev, shuffle=False):
        cmap, mask = steps.infer_density(netS, x, y, prob_thresh)
        maskf = mask.to(cmap.dtype)
        valid = torch.zeros_like(mask)
        items = item.tolist()[:real]                       # padded duplicates belong to another rank
        for i, it in enumerate(items):
            r0, r1, c0, c1 = grid.eff_range(it)
            valid[i, :, r0:r1, c0:c1] = True
        if ds.ref is not None:
            acc.add_batch_map(r, maskf, gt_map, pre_map, valid=valid)
            codes = metrics.changemap_codes(maskf, r, True, ref_map=gt_map, dt_map=pre_map)
        else:
            codes = metrics.changemap_codes(maskf, maskf, False, dt_map=pre_map)
        cm_h, co_h = cmap.cpu().numpy(), codes.cpu().numpy()
        for i, it in enumerate(items):
            grid.write_center(density, cm_h[i], it)
            grid.write_center(color, co_h[i], it)
    if dp.exchanging():
        both = torch.from_numpy(np.stack([density, color])).to(dev)
        dp.sum_counts(both)
        density, color = (a.copy() for a in both.cpu().numpy())
    netS.train(was_training)
    return dict(density=density, color=color, evaluator=acc)


@torch.no_grad()
def infer_scene_resident(netS, scene, device, batch_size=10, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1), eval_mode=True,
                         raw=False):
    """``infer_scene`` with everything but the network's weights of the loop kept on the device: ``scene`` is a
    ``tiles.ResidentScene`` (single scene); tiles are cut by ``fcd_scene_cut``, the owned centres written into device maps,
    colour-coded and counted by ``fcd_scene_stitch`` -- two launches per batch around the Segmentor, no host tile loop, ONE
    device-to-host copy per map at the end.  Same batches as ``infer_scene`` (``dp.RankStridedBatches(shuffle=False)``, padded
    duplicates cut and inferred but not stitched), same data-parallel rule (each rank stitches its own tiles into zeroed maps,
    maps and counts are summed across ranks on the device), same returned dict -- bit for bit, since the input tiles are.
    ``raw=True`` cuts plain samples and runs ``steps.infer_density_raw`` (NORMALIZE folded into the first convolution): eval
    mode only, density within rounding of the normalised path."""
    if not isinstance(scene, tiles.ResidentScene):
        raise TypeError('infer_scene_resident takes a tiles.ResidentScene (one scene pair), got %s' % type(scene).__name__)
    if raw and not eval_mode:
        raise RuntimeError('raw=True folds NORMALIZE into the first convolution: eval mode only (Segmentor.forward_raw)')
    if raw and scene.stats is None:
        raise RuntimeError('raw=True needs the scene statistics (ResidentScene(stats=...))')
    from . import _ops as ops
    dev = torch.device(device)
    if eval_mode:
        dp.sync_buffers((netS,))
    was_training = netS.training
    netS.train(not eval_mode)
    grid = scene.grid
    density, color = scene.new_maps()
    acc = metrics.Evaluator(2)
    counts = acc.device_counts(dev) if scene.ref is not None else None
    sampler = dp.RankStridedBatches(len(grid), batch_size, seed=0, shuffle=False)
    for b, items in enumerate(sampler):
        real = len(items) - sampler.pads[b]                    # padded duplicates belong to another rank
        table = ops.scene_tile_table(grid, items)
        x, y, _, valid = scene.cut(table, raw=raw)
        if raw:
            cmap, _ = steps.infer_density_raw(netS, x, y, valid, scene.stats, prob_thresh)
        else:
            cmap, _ = steps.infer_density(netS, x, y, prob_thresh)
        if real > 0:
            ops.scene_stitch(cmap, table, density, color, n=real, prob_thresh=prob_thresh, gt_map=gt_map, pre_map=pre_map,
                             write_color=True, ref=scene.ref, counts=counts)
    if dp.exchanging():
        both = torch.stack([density, color])
        dp.sum_counts(both)                                    # the evaluator's counts are summed in Evaluator._sync
        density, color = both[0], both[1]
    netS.train(was_training)
    return dict(density=density.cpu().numpy(), color=color.cpu().numpy(), evaluator=acc)


def _set_result(names, density, color, scene_counts, has_ref, acc=None):
    """The dict both set routes return.  ``scene_counts``: (S,4) int64 device counter (row s = scene s) or None; the
    per-scene evaluators take its rows without a copy, the overall one their sum; a scene without a reference has no counts."""
    scene_acc = None
    if scene_counts is not None:
        scene_acc = [metrics.Evaluator(2) for _ in names]
        for s, ev in enumerate(scene_acc):
            if has_ref[s]:
                ev.attach_counts(scene_counts[s])
        acc = metrics.Evaluator(2)
        if any(has_ref):
            acc.attach_counts(scene_counts.sum(0))
    return dict(density=density, color=color, evaluator=acc, scene_evaluators=scene_acc, names=list(names))


def _no_ref_scores_nothing(has_ref, gt_map):
    # a scene without a reference gives zero reference tiles: they must not land in a cell
    if not all(has_ref) and any(float(g) == 0.0 for g in gt_map):
        raise ValueError('score_only: a scene without a reference map in a set scored against gt_map %r (0 is a class)' % (gt_map,))


@torch.no_grad()
def infer_scene_set(netS, ds, device, batch_size=10, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1), eval_mode=True,
                    score_only=False):
    """``infer_scene`` over a ``datasets.MultiSceneDataset``: the reference's test pass and final maps over SEVERAL scenes
    (Demo_RSSS.py:399-447,451-502).  The tiles are walked in global item order without shuffling, so a batch may hold tiles of
    two scenes -- with ``eval_mode=False`` (the per-epoch test pass: BatchNorm in train mode) the batch composition is part of
    the result, which is why this is not a loop of ``infer_scene`` calls.  Returns ``dict(density=[(1,H,W) per scene],
    color=[...], evaluator=<overall>, scene_evaluators=[per scene], names=...)``; a scene without a reference map gets the
    detection-only colour code and counts nothing.  ``score_only=True``: counts only (``add_batch_map`` over the owned
    centres): no maps (``density`` / ``color`` None) and no per-scene evaluators.  Data parallel: as ``infer_scene``."""
    if not isinstance(ds, datasets.MultiSceneDataset):
        raise TypeError('infer_scene_set takes a datasets.MultiSceneDataset, got %s' % type(ds).__name__)
    dev = torch.device(device)
    if eval_mode:
        dp.sync_buffers((netS,))
    was_training = netS.training
    netS.train(not eval_mode)
    S = len(ds.scenes)
    has_ref = [s.ref is not None for s in ds.scenes]
    if score_only:
        _no_ref_scores_nothing(has_ref, gt_map)
    density, color = (None, None) if score_only else (ds.new_outputs(), ds.new_outputs())
    acc = metrics.Evaluator(2)
    acc.device_counts(dev)                                  # allocated on every rank: the collectives stay in step
    scene_counts = None if score_only else torch.zeros((S, 4), dtype=torch.int64, device=dev)
    for batch, real, _ in _Epoch(ds, batch_size, 0, dev, shuffle=False):
        x, y, item, r = batch[:4]
        cmap, mask = steps.infer_density(netS, x, y, prob_thresh)
        maskf = mask.to(cmap.dtype)
        items = item.tolist()[:real]                        # padded duplicates belong to another rank
        scene_of = [ds.locate(it)[0] for it in items]
        valid = torch.zeros_like(mask, dtype=torch.bool)
        for i, it in enumerate(items):
            if has_ref[scene_of[i]]:
                r0, r1, c0, c1 = ds.eff_range(it)
                valid[i, :, r0:r1, c0:c1] = True
        if score_only:
            acc.add_batch_map(r, maskf, gt_map, pre_map, valid=valid)
            continue
        for s in sorted(set(scene_of)):
            if has_ref[s]:
                ev = metrics.Evaluator(2)
                mine = _rows_mask(valid, [i for i, k in enumerate(scene_of) if k == s])
                ev.add_batch_map(r, maskf, gt_map, pre_map, valid=valid & mine)
                scene_counts[s] += ev._dev_counts
        codes = metrics.changemap_codes(maskf, r, True, ref_map=gt_map, dt_map=pre_map)
        plain = metrics.changemap_codes(maskf, maskf, False, dt_map=pre_map)
        with_ref = _rows_mask(valid, [i for i, k in enumerate(scene_of) if has_ref[k]])
        codes = torch.where(with_ref, codes, plain)
        cm_h, co_h = cmap.cpu().numpy(), codes.cpu().numpy()
        for i, it in enumerate(items):
            ds.write_center(density, cm_h[i], it)
            ds.write_center(color, co_h[i], it)
    if not score_only and dp.exchanging():
        sizes = [d.size for d in density]
        both = torch.from_numpy(np.concatenate([d.ravel() for d in density + color])).to(dev)
        dp.sum_counts(both)
        flat = np.split(both.cpu().numpy(), np.cumsum(sizes + sizes)[:-1])
        density = [f.reshape(d.shape).copy() for f, d in zip(flat[:S], density)]
        color = [f.reshape(d.shape).copy() for f, d in zip(flat[S:], density)]
    netS.train(was_training)
    return _set_result(ds.names, density, color, scene_counts, has_ref, acc)


def _rows_mask(like, rows):
    """(N,1,1,1) bool on ``like``'s device: True for the tiles ``rows`` of the batch."""
    m = torch.zeros((like.shape[0], 1, 1, 1), dtype=torch.bool, device=like.device)
    if rows:
        m[rows] = True
    return m


@torch.no_grad()
def infer_scene_set_resident(netS, scene_set, device, batch_size=10, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1),
                             eval_mode=True, score_only=False):
    """``infer_scene_set`` with the data path on the device: ``scene_set`` is a ``tiles.ResidentSceneSet``.  Same batches
    (``dp.RankStridedBatches(shuffle=False)`` over the global items, so tiles of different scenes share a batch), the index
    list uploaded ONCE; per batch one ``fcd_scene_set_cut`` and one ``fcd_scene_set_stitch`` around the Segmentor, which writes
    every tile into its own scene's maps and counts it into its own scene's row; at the end ONE device-to-host copy per flat
    map.  Same returned dict, bit for bit.  ``score_only=True``: no maps; the counts come from ``Evaluator.add_tiles`` on the
    resident rectangles of the set.  Data parallel: each rank stitches its tiles into zeroed maps, the two flat buffers are
    summed with one ``dp.sum_counts`` and the counters are all-reduced when the scores are read.  There is no ``raw=True``
    route: the statistics differ per tile of a batch, so NORMALIZE cannot be folded into the first convolution."""
    if not isinstance(scene_set, tiles.ResidentSceneSet):
        raise TypeError('infer_scene_set_resident takes a tiles.ResidentSceneSet, got %s' % type(scene_set).__name__)
    dev = scene_set.device
    if eval_mode:
        dp.sync_buffers((netS,))
    was_training = netS.training
    netS.train(not eval_mode)
    S = len(scene_set.scenes)
    has_ref = [s.ref is not None for s in scene_set.scenes]
    if score_only:
        _no_ref_scores_nothing(has_ref, gt_map)
    acc = metrics.Evaluator(2)
    acc.device_counts(dev)
    maps = None if score_only else scene_set.new_maps()
    scene_counts = None if score_only else torch.zeros((S, 4), dtype=torch.int64, device=dev)
    plan = tiles.EpochPlan(len(scene_set), batch_size, 0, shuffle=False)
    index = scene_set.index(plan.flat) if plan.flat else None
    for b, items in enumerate(plan.batches):
        part = index[plan.offsets[b]:plan.offsets[b + 1]]
        real = len(items) - plan.pads[b]                    # padded duplicates belong to another rank
        x, y, r, _, _ = scene_set.cut(part, want_valid=False)
        cmap, _ = steps.infer_density(netS, x, y, prob_thresh)
        if real <= 0:
            continue
        if score_only:
            acc.add_tiles(r, cmap, scene_set.rects(part, real), prob_thresh, gt_map, pre_map)
        else:
            scene_set.stitch(cmap, part, maps, n=real, prob_thresh=prob_thresh, gt_map=gt_map, pre_map=pre_map,
                             write_color=True, scene_counts=scene_counts)
    density = color = None
    if not score_only:
        if dp.exchanging():
            both = torch.stack([maps.flat_density, maps.flat_color])
            dp.sum_counts(both)
        else:
            both = (maps.flat_density, maps.flat_color)
        off = scene_set.table.offsets
        flat_d, flat_c = both[0].cpu().numpy(), both[1].cpu().numpy()       # ONE copy per flat map
        shapes = [(1, h, w) for w, h in scene_set.table.sizes]
        density = [flat_d[off[s]:off[s + 1]].reshape(shapes[s]) for s in range(S)]
        color = [flat_c[off[s]:off[s + 1]].reshape(shapes[s]) for s in range(S)]
    netS.train(was_training)
    return _set_result(scene_set.names, density, color, scene_counts, has_ref, acc)


def _scores(ev):
    """The seven scores the reference logs per test pass (Demo_RSSS.py:432-447) as a dict of floats."""
    miou, ciou = ev.Mean_Intersection_over_Union()
    return dict(OA=float(ev.Pixel_Accuracy()), Kappa=float(ev.Pixel_Kappa()), precision=float(ev.Pixel_Precision_Rate()),
                recall=float(ev.Pixel_Recall_Rate()), F1=float(ev.Pixel_F1_score()), mIoU=float(miou), cIoU=float(ciou))


def _valid_centres(dataset, like, items, real):
    valid = torch.zeros_like(like, dtype=torch.bool)
    for i, it in enumerate(items[:real]):
        r0, r1, c0, c1 = dataset.eff_range(it) if hasattr(dataset, 'eff_range') else dataset.grid.eff_range(it)
        valid[i, :, r0:r1, c0:c1] = True
    return valid


def demo_rsss(dataset, device='cuda', n_channels=4, epochs_g=50, epochs_adv=100, init_batch_size=20, batch_size=12,
              learning_rate=5e-5, perception_weight=0.1, ssim_weight=0, perception_perBand=True, l1_weight=0.02,
              g_weight=0.5, d_weight=1, r_weight=2, prob_thresh=0.5, gt_map=(1, 2), pre_map=(0, 1), seed=0,
              netG_state=None, log=None, allow_seeded=False, load_g=None, save_s=None, save_g=None, save_d=None, ragged='pad',
              region_from_ref=None, test_dataset=None, test_batch_size=None, out_dir=None):
    """Demo_RSSS.py:27-538 on a ``datasets.MultiSceneDataset`` / ``RegionTileDataset`` (tuples
    ``(x, y, item, ref, region)``): G pre-training on the region-masked reconstruction (skipped when a
    generator checkpoint is given -- ``load_g``: path of a ``GModel.pkl`` as the reference writes it,
    Demo_RSSS.py:167-171, or ``netG_state``: a state_dict), netG.eval(), adversarial D/S loop with the
    reference's LR schedules, per-epoch on-device accuracy over the owned tile centres, ``.pkl`` checkpoints
    (``save_s/save_g/save_d``, Demo_RSSS.py:507-514).  Batch sizes are per rank under data parallelism.
    ``dataset`` may be a ``tiles.ResidentSceneSet`` (scenes with region maps, resident on the device): the same batches are
    then cut on the device (``ResidentSceneSet.epoch``) and the accuracy is one ``Evaluator.add_tiles`` call per batch on
    resident rectangles -- no host work per tile, no copy per batch.  ``region_from_ref=(thresh, expand)``: a resident scene that
    has a reference map but no region map gets one derived from it on the device (``ResidentScene.derive_region``: what
    OSCDProcess.py:56-73 prepares offline; OSCD's recipe is ``(1, 10)``); the default None keeps the error.
    ``test_dataset``: a ``tiles.ResidentSceneSet`` or a ``datasets.MultiSceneDataset`` of several scenes, held either way
    whatever the training set is (``infer_scene_set_resident`` / ``infer_scene_set``; batches of ``test_batch_size``, default
    ``batch_size``).  After every adversarial epoch it is scored as the reference does (Demo_RSSS.py:399-447): counts only, under
    ``no_grad`` (same values, no tape) and with ``netS`` in TRAIN mode as there -- so the BatchNorm running statistics of
    ``netS`` move with the test batches, and the tiles of a batch, which may belong to two scenes, are normalised together.
    ``history['test']`` gets one dict per epoch: OA, Kappa, precision, recall, F1, mIoU, cIoU.  After the last epoch and the
    buffer broadcast a full eval-mode pass makes the per-scene density and colour maps (Demo_RSSS.py:451-502): its result is
    returned under ``test``, and with ``out_dir`` rank 0 writes ``<name>_density.tif`` and ``<name>_binary.tif`` per scene.
    Without ``test_dataset`` nothing of this happens and the returned dict has no ``test`` key."""
    dev = torch.device(device)
    resident = isinstance(dataset, tiles.ResidentSceneSet)
    test_pass = None
    if test_dataset is not None:
        if isinstance(test_dataset, tiles.ResidentSceneSet):
            test_route = infer_scene_set_resident
        elif isinstance(test_dataset, datasets.MultiSceneDataset):
            test_route = infer_scene_set
        else:
            raise TypeError('test_dataset: a tiles.ResidentSceneSet or a datasets.MultiSceneDataset, got %s'
                            % type(test_dataset).__name__)
        test_pass = lambda **kw: test_route(netS, test_dataset, dev, batch_size=test_batch_size or batch_size,
                                            prob_thresh=prob_thresh, gt_map=gt_map, pre_map=pre_map, **kw)
    if resident:
        if region_from_ref is not None:
            todo = [s for s in dataset.scenes if s.region is None and s.ref is not None]
            for s in todo:
                s.derive_region(region_from_ref[0], region_from_ref[1])
            if todo:
                dataset.refresh()
        if not dataset.has_region:
            raise ValueError('demo_rsss needs region maps: ResidentScene(..., region=...)')
        epoch = lambda bs, sd: dataset.epoch(bs, sd, ragged=ragged)
    else:
        epoch = lambda bs, sd: _Epoch(dataset, bs, sd, dev, ragged=ragged)
    torch.manual_seed(seed)
    netD = Module.Discriminator_SRGAN_simple(n_channels=n_channels).to(dev)
    netS = Module.Segmentor(n_channels=n_channels, bilinear=True).to(dev)
    netG = Module.Generator(n_channels=n_channels).to(dev)
    netS.train(); netG.train(); netD.train()
    crit = Loss.CGeneratorLoss(channel=n_channels, perception_layer=1, perception_perBand=perception_perBand,
                               allow_seeded=allow_seeded).to(dev)
    optG = optim.Adam(netG.parameters(), lr=learning_rate, betas=(0.9, 0.99))
    optS = optim.RMSprop(netS.parameters(), lr=learning_rate)
    optD = optim.RMSprop(netD.parameters(), lr=learning_rate)
    hist = {'g': [], 'adv': []}
    if load_g is not None and os.path.exists(load_g):                            # Demo_RSSS.py:167-171
        netG_state = torch.load(load_g, map_location=dev)
    if netG_state is not None:
        netG.load_state_dict(netG_state)
        epochs_g = 0
    dp.sync_start((netS, netD, netG), (optS, optD, optG))
    for ep in range(epochs_g):                                                   # Demo_RSSS.py:175-236
        optim.adjust_learning_rate(optG, ep, lr_start=1e-5, lr_max=3e-4, lr_warm_up_epoch=10, lr_sustain_epochs=10)
        tot = torch.zeros((), device=dev)
        for (x, y, item, r, region), real, w in epoch(init_batch_size, seed * 1000 + ep):
            out = steps.rsss_g_pretrain_step(netG, crit, optG, x, y, region, perception_weight, ssim_weight, loss_scale=w.loss_scale)
            tot += out['g_loss'].detach() * w
        hist['g'].append(float(_epoch_mean(tot)))
        if log:
            log('G pre-train epoch %d g_loss %.4f' % (ep + 1, hist['g'][-1]))
    netG.eval()                                                                   # Demo_RSSS.py:240
    acc = metrics.Evaluator(2)
    for ep in range(epochs_adv):                                                  # Demo_RSSS.py:246-396
        optim.adjust_learning_rate(optS, ep, lr_start=1e-4, lr_max=1e-3, lr_warm_up_epoch=5)
        optim.adjust_learning_rate(optD, ep, lr_start=5e-6, lr_max=5e-5, lr_min=5e-7, lr_warm_up_epoch=5)
        acc.reset()
        sums = torch.zeros(3, device=dev)
        for (x, y, item, r, region), real, w in epoch(batch_size, seed * 1000 + 500 + ep):
            out = steps.rsss_adversarial_step(netS, netD, netG, crit, optS, optD, x, y, region,
                                              perception_weight=perception_weight, ssim_weight=ssim_weight,
                                              l1_weight=l1_weight, g_weight=g_weight, d_weight=d_weight,
                                              r_weight=r_weight, loss_scale=w.loss_scale)
            sums += torch.stack([out['d_loss'].detach(), out['s_loss'].detach(), out['g_loss'].detach()]) * w
            if resident:
                if w.rects is not None:
                    acc.add_tiles(r, out['cmap'].detach(), w.rects, prob_thresh, gt_map, pre_map)
                continue
            valid = _valid_centres(dataset, out['cmap'], item.tolist(), real)
            acc.add_batch_map(r, metrics.threshold_map(out['cmap'].detach(), prob_thresh), gt_map, pre_map, valid=valid)
        hist['adv'].append([float(v) for v in _epoch_mean(sums)] + [float(acc.Pixel_F1_score())])
        if log:
            log('adv epoch %d d %.4f s %.4f g %.4f F1 %.4f' % ((ep + 1,) + tuple(hist['adv'][-1])))
        if test_pass is not None:                                                 # Demo_RSSS.py:399-447: netS stays in train mode
            hist.setdefault('test', []).append(_scores(test_pass(eval_mode=False, score_only=True)['evaluator']))
            if log:
                log('adv epoch %d test F1 %.4f' % (ep + 1, hist['test'][-1]['F1']))
    dp.sync_buffers((netS, netG, netD))      # the saved .pkl = the statistics every rank infers with from here on
    _save(netS, save_s)
    _save(netG, save_g)
    _save(netD, save_d)
    res = dict(netS=netS, netD=netD, netG=netG, history=hist, evaluator=acc, vgg_pretrained=crit.loss_perception.pretrained)
    if test_pass is not None:                                                     # Demo_RSSS.py:451-502
        hist.setdefault('test', [])
        res['test'] = test = test_pass(eval_mode=True)
        if out_dir and dp.world_info()[0] == 0:
            os.makedirs(out_dir, exist_ok=True)
            for name, den, col in zip(test['names'], test['density'], test['color']):
                tiles.write_tiff(os.path.join(out_dir, '%s_density.tif' % name), den)
                tiles.write_tiff(os.path.join(out_dir, '%s_binary.tif' % name), col)
    return res


def demo_wsss(changed_ds, unchanged_ds, device='cuda', n_channels=3, epochs_g=50, epochs_adv=50, unc_batch_size=50,
              batch_size=15, perception_weight=0.5, ssim_weight=0, g_weight=0.2, l1_weight=1.6, d_weight=1,
              nc_weight=1.5, seed=0, netG_state=None, log=None, allow_seeded=False, load_g=None, save_s=None,
              save_g=None, save_d=None, ragged='pad'):
    """Demo_WSSS.py:27-483 on datasets of (x, y, ...) tuples: G pre-training on UNCHANGED pairs
    with cmap = 0 (Demo_WSSS.py:152-176; skipped with ``load_g`` / ``netG_state``, :131-135), netG.eval(),
    adversarial loop over (changed, unchanged) pairs re-matched every epoch (``PairingDataset.order_reset``,
    same seed on every rank), ``.pkl`` checkpoints (:454-461)."""
    from .datasets import PairingDataset
    dev = torch.device(device)
    torch.manual_seed(seed)
    netD = Module.Discriminator_SRGAN_simple(n_channels).to(dev)
    netS = Module.Segmentor(n_channels=n_channels, bilinear=True).to(dev)
    netG = Module.Generator(n_channels=n_channels).to(dev)
    netS.train(); netD.train(); netG.train()
    crit = Loss.CGeneratorLoss(channel=n_channels, perception_layer=1, perception_perBand=False,
                               allow_seeded=allow_seeded).to(dev)
    optG = optim.Adam(netG.parameters(), lr=5e-4, betas=(0.9, 0.99))
    optS = optim.RMSprop(netS.parameters(), lr=1e-3)
    optD = optim.RMSprop(netD.parameters(), lr=1e-5)
    hist = {'g': [], 'adv': []}
    if load_g is not None and os.path.exists(load_g):                            # Demo_WSSS.py:131-135
        netG_state = torch.load(load_g, map_location=dev)
    if netG_state is not None:
        netG.load_state_dict(netG_state)
        epochs_g = 0
    if g_weight == 0:
        epochs_g = 0
    dp.sync_start((netS, netD, netG), (optS, optD, optG))
    for ep in range(epochs_g):
        optim.adjust_learning_rate(optG, ep, lr_start=1e-5, lr_max=3e-4, lr_warm_up_epoch=10, lr_sustain_epochs=10)
        tot = torch.zeros((), device=dev)
        for batch, real, w in _Epoch(unchanged_ds, unc_batch_size, seed * 1000 + ep, dev, ragged=ragged):
            x, y = batch[0], batch[1]
            optG.zero_grad()
            y_fake = netG(x)
            cmap = torch.zeros((x.shape[0], 1, x.shape[2], x.shape[3]), device=dev)
            gen, ssim, perc = crit(y, y_fake, cmap)
            g_loss = gen + perception_weight * perc + ssim_weight * ssim
            optG.begin_overlap()
            steps._backward(g_loss, w.loss_scale)
            optG.allreduce_grads()
            optG.step()
            tot += g_loss.detach() * w
        hist['g'].append(float(_epoch_mean(tot)))
        if log:
            log('G pre-train epoch %d g_loss %.4f' % (ep + 1, hist['g'][-1]))
    netG.eval()                                                                   # Demo_WSSS.py:206
    pairs = PairingDataset(changed_ds, unchanged_ds, random_assign=False, seed=seed)

    def flat(loader):
        for cds, ncds in loader:
            yield (cds[0], cds[1], ncds[0], ncds[1])
    for ep in range(epochs_adv):                                                  # Demo_WSSS.py:209-323
        optim.adjust_learning_rate(optS, ep, lr_start=1e-4, lr_max=1e-3, lr_warm_up_epoch=5)
        optim.adjust_learning_rate(optD, ep, lr_start=1e-6, lr_max=1e-5, lr_min=1e-8, lr_warm_up_epoch=5)
        pairs.order_reset(seed=seed * 7919 + ep)                                   # same pairing on every rank
        sums = torch.zeros(2, device=dev)
        for (x, y, x_nc, y_nc), real, w in _Epoch(pairs, batch_size, seed * 1000 + 700 + ep, dev, wrap=flat, ragged=ragged):
            out = steps.wsss_adversarial_step(netS, netD, netG, crit, optS, optD, x, y, x_nc, y_nc,
                                              perception_weight=perception_weight, ssim_weight=ssim_weight,
                                              g_weight=g_weight, l1_weight=l1_weight, d_weight=d_weight,
                                              nc_weight=nc_weight, loss_scale=w.loss_scale)
            sums += torch.stack([out['d_loss'].detach(), out['s_loss'].detach()]) * w
        hist['adv'].append([float(v) for v in _epoch_mean(sums)])
        if log:
            log('adv epoch %d d %.4f s %.4f' % ((ep + 1,) + tuple(hist['adv'][-1])))
    dp.sync_buffers((netS, netG, netD))
    _save(netS, save_s)
    _save(netG, save_g)
    _save(netD, save_d)
    return dict(netS=netS, netD=netD, netG=netG, history=hist, vgg_pretrained=crit.loss_perception.pretrained)
