# -*- coding: utf-8 -*-
"""TorchRecSys — drop-in for the reference's torchrecsys.model.TorchRecSys (reference model.py:18-452) whose
fit() / evaluate() / predict() run on hand-written HIP kernels on the MI355X.

Same constructor keywords, same methods, same printed strings, same state_dict keys.  Extra keywords (superset API):
  hidden_layers, use_batch_norm : reach the MLP (the reference advertises them but cannot pass them)
  rng : 'reference' (default) replays the reference's host RNG streams (torch.randperm shuffle, numpy legacy sampler) so
        a seeded run sees bit-identical batches;  'device' keeps the whole interaction stream in HBM and shuffles /
        samples on the GPU with counter-based generators (same distributions, different streams) — the mode the
        benchmark runs in
  seed : seed of the device-side generators (rng='device')
"""
import collections
import functools
import math
import os
from collections.abc import Mapping
from typing import List

import numpy as np
import pandas as pd
import torch
import torch.profiler

from . import dist as tdist
from . import ops
from .collaborative._scorer import check_err_flag
from .collaborative.fm import FM
from .collaborative.linear import Linear
from .dataset.dataset import FastDataLoader, ProcessData, sample_negatives_reference_stream
from .engine import SparseScorerTrainer
from .evaluate import diversity as diversity_eval
from .evaluate import ranks as rank_eval
from .evaluate.metrics import Metrics
from .helper.cuda import gpu, host_threads
from .helper.loss import hinge_loss  # noqa: F401  (part of the reference's module surface)


def _host_side(fn):
    """Run a public entry point under helper.cuda.host_threads() (torch's CPU thread pool capped at the CPU budget)."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with host_threads():
            return fn(*args, **kwargs)
    return wrapped

_NO_GPU_MSG = ("torchrecsys_amd needs an AMD Instinct MI355X (gfx950) visible to PyTorch-ROCm; "
               "it has no CPU fallback (use_cuda=False only means: hand results back as CPU tensors)")


def _device():
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU_MSG)
    return torch.device("cuda", torch.cuda.current_device())


def _mix64(a, b):
    """SplitMix64-style hash of two integers -> 64-bit key (device shuffle / sampler keys per epoch)."""
    x = (a * 0x9E3779B97F4A7C15 + b + 0x632BE59BD9B4E019) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 31
    return x or 1


def _check_mining_options(ns, net_type):
    """The score-aware mining keys of neg_sampling (fit() docstring): ValueError naming the offending key."""
    if ns.get("mine") is None:
        for key in ("candidates", "top"):
            if key in ns:
                raise ValueError(f"neg_sampling[{key!r}] needs neg_sampling['mine'] (= 'hardest')")
        if "mine" in ns:
            raise ValueError("neg_sampling['mine'] must be 'hardest'")
        return
    if ns["mine"] != 'hardest':
        raise ValueError(f"neg_sampling['mine'] must be 'hardest', got {ns['mine']!r}")
    if net_type not in ('linear', 'fm'):
        raise ValueError("neg_sampling['mine'] scores every candidate with the Linear / FM kernels; a candidate's score "
                         f"under net_type={net_type!r} needs the whole network (out of scope)")

    def integer(key, default, lo, hi):
        v = ns.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError(f"neg_sampling[{key!r}] must be an integer in {lo}..{hi}, got {v!r}")
        return int(v)

    K = integer("candidates", 8, 1, 64)
    integer("top", 1, 1, K)


def _check_l2(l2, net_type):
    """fit(l2=...): None when every coefficient is 0, else (lambda_user, lambda_item, lambda_metadata)."""
    groups = ('user', 'item', 'metadata')

    def number(v, what):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{what} must be a non-negative finite number, got {v!r}")
        v = float(v)
        if not (math.isfinite(v) and v >= 0):
            raise ValueError(f"{what} must be a non-negative finite number, got {v!r}")
        return v

    if isinstance(l2, Mapping):
        for key in l2:
            if key not in groups:
                raise ValueError(f"l2 has the unknown key {key!r}: its keys are among {groups}")
        lam = tuple(number(l2.get(g, 0.0), f"l2[{g!r}]") for g in groups)
    else:
        lam = (number(l2, "l2"),) * 3
    if not any(lam):
        return None
    if net_type not in ('linear', 'fm'):
        raise ValueError("l2 regularises the embedding rows of the Linear and FM scorers (net_type 'linear' or 'fm'): "
                         f"with net_type={net_type!r} the dense layers take the optimiser's own weight_decay, and its "
                         "embedding rows are not covered")
    return lam


def ordered_sequences(users, items, rows, n_users, timestamps=None):
    """The ordered per-user CSR of a set of interactions (fit_sequence): users / items (n,) dense ids, rows (n,) the
    distinct input position of each interaction, timestamps None or one value per INPUT row (indexed by `rows`).
    Returns (offsets int64 (n_users + 1,), item ids int32 (n,)): user u's items in ascending (timestamp, input
    position), repeated items kept.  Runs where the tensors live (three stable sorts)."""
    users = users.to(torch.int64)
    order = torch.argsort(rows, stable=True)
    if timestamps is not None:
        ts = timestamps[rows]
        order = order[torch.argsort(ts[order], stable=True)]
    order = order[torch.argsort(users[order], stable=True)]
    off = torch.zeros(int(n_users) + 1, dtype=torch.int64, device=users.device)
    off[1:] = torch.cumsum(torch.bincount(users, minlength=int(n_users)), 0)
    return off, items[order].to(torch.int32).contiguous()


def sequence_entries(off, holdout_last):
    """The positions of an ordered CSR that fit_sequence trains on: all of them, or with holdout_last all but the last
    of every row with at least two.  Returns (entries int64, held-out users int64, held-out positions int64)."""
    n = int(off[-1])
    entries = torch.arange(n, dtype=torch.int64, device=off.device)
    if not holdout_last:
        return entries, entries[:0], entries[:0]
    has = (off[1:] - off[:-1]) >= 2
    held_users = torch.nonzero(has).reshape(-1)
    held_pos = off[1:][has] - 1
    keep = torch.ones(n, dtype=torch.bool, device=off.device)
    keep[held_pos] = False
    return entries[keep], held_users, held_pos


# What fit() trains on, as its validation chose it: kind 'pair' (hinge / bpr on one negative) | 'softmax' (in-batch) |
# 'multineg' (K sampled negatives) | 'warp'; loss_id the pair loss (_lib.LOSS_ID) of 'pair' and of 'multineg' (there
# also _lib.LOSS_SAMPLED_SOFTMAX); logq the (n_items,) device table or None; rank_weight 'log' | 'harmonic'
Objective = collections.namedtuple("Objective", "kind loss_id K temperature logq margin rank_weight")


class TorchRecSys(torch.nn.Module):
    _objective = Objective('pair', 0, 1, 1.0, None, 1.0, 'log')  # never fitted: evaluate() reports the hinge loss

    @_host_side
    def __init__(self,
                 dataset: pd.DataFrame,
                 user_id_col: str,
                 item_id_col: str,
                 n_factors: int = 80,
                 net_type: str = 'linear',
                 metadata_id_col: List[str] = None,
                 split_ratio: float = 0.8,
                 dynamic_neg_sampling: bool = False,
                 use_amp: bool = False,
                 use_cuda: bool = False,
                 debug: bool = False,
                 path: str = './',
                 hidden_layers: List[int] = None,
                 use_batch_norm: bool = True,
                 rng: str = 'reference',
                 seed: int = 0,
                 neg_sampling: dict = None):
        super().__init__()
        self.neg_sampling = neg_sampling
        data_processor = ProcessData(dataset=dataset, user_id_col=user_id_col, item_id_col=item_id_col,
                                     metadata_id_col=metadata_id_col, split_ratio=split_ratio,
                                     dynamic_neg_sampling=dynamic_neg_sampling)
        self._setup(data_processor, metadata_id_col, n_factors, net_type, dynamic_neg_sampling, use_amp, use_cuda,
                    debug, path, hidden_layers, use_batch_norm, rng, seed)

    @classmethod
    def from_tensors(cls, user_ids, item_ids, n_users=None, n_items=None, item_metadata=None, metadata_names=None,
                     n_factors=80, net_type='linear', split_ratio=0.8, dynamic_neg_sampling=False, use_amp=False,
                     use_cuda=False, debug=False, path='./', hidden_layers=None, use_batch_norm=True, rng=None,
                     seed=0, pre_sharded=False, dp_partition='user', remap_ids=False, split=None, neg_sampling=None):
        """Tensor-native ingest (no DataFrame): id tensors on the CPU or already in HBM.  GPU tensors default to
        rng='device' (stream resident in HBM, on-device shuffle and sampler).  pre_sharded=True: under data parallelism
        the given interactions already ARE this rank's shard (each rank ingested its own part), so they are not cut
        again by rank; shards may differ in length (every rank then trains on the common number of rows, see
        _rank_rows).  dp_partition: how the stream is (pre_sharded: was) cut — 'user' = by user_id % world (each user
        row has ONE writer, see fit()), 'contiguous' = equal contiguous blocks.  remap_ids / split: see
        dataset.TensorProcessData (dense re-mapping of arbitrary ids; 'reference' = the reference's RandomState(42)
        split also for GPU tensors, 'device' = a seeded permutation drawn on the GPU)."""
        from .dataset.dataset import TensorProcessData
        self = cls.__new__(cls)
        torch.nn.Module.__init__(self)
        self.neg_sampling = neg_sampling
        dp = TensorProcessData(user_ids, item_ids, n_users, n_items, item_metadata, metadata_names, split_ratio,
                               dynamic_neg_sampling, remap_ids=remap_ids, split=split)
        if rng is None:
            rng = 'device' if user_ids.is_cuda else 'reference'
        if user_ids.is_cuda and rng != 'device':
            raise ValueError("GPU-resident id tensors require rng='device'")
        self._setup(dp, dp.metadata_id_col, n_factors, net_type, dynamic_neg_sampling, use_amp, use_cuda, debug, path,
                    hidden_layers, use_batch_norm, rng, seed)
        self.pre_sharded = bool(pre_sharded)
        assert dp_partition in ('user', 'contiguous')
        self.dp_partition = dp_partition
        return self

    def _setup(self, data_processor, metadata_id_col, n_factors, net_type, dynamic_neg_sampling, use_amp, use_cuda,
               debug, path, hidden_layers, use_batch_norm, rng, seed):
        assert rng in ('reference', 'device'), 'rng must be "reference" or "device"'
        ns = getattr(self, "neg_sampling", None)
        if ns:
            unknown = set(ns) - {"reject_seen", "popularity", "k", "max_tries", "mine", "candidates", "top"}
            if unknown or rng != 'device' or not dynamic_neg_sampling:
                raise ValueError("neg_sampling takes reject_seen / popularity / k / max_tries / mine / candidates / top "
                                 "and needs rng='device' with dynamic_neg_sampling=True (the reference-RNG mode replays "
                                 "the reference's sampler)")
            _check_mining_options(ns, net_type)
        self.path = path
        self.dynamic_neg_sampling = dynamic_neg_sampling
        self.use_amp = use_amp
        self.use_cuda = use_cuda
        self.rng = rng
        self.seed = seed
        self.grad_scaler = None  # bf16 GEMM inputs with fp32 accumulation need no loss scaling
        self.data_processor = data_processor
        self.data_processor.prepare_data()
        self.config = self.data_processor.config
        self.n_users = self.config.get('num_users')
        self.n_items = self.config.get('num_items')
        self.metadata_size = self.config.get('num_metadata')
        self.metadata_name = metadata_id_col if getattr(self.data_processor, 'metadata_id_col', None) else None
        self.n_factors = n_factors
        self.net_type = net_type
        self.use_metadata = True if self.metadata_name else False
        self.debug = debug
        self.hidden_layers = hidden_layers
        self.use_batch_norm = use_batch_norm
        self._fit_epochs_done = 0
        self._dev_cache = {}
        self.dp_partition = 'user'  # data-parallel cut of the interaction stream (fit() docstring)
        self._init_net(net_type=net_type)

    # ------------------------------------------------------------------------------------------------ net
    def _init_net(self, net_type='linear'):
        assert net_type in ('linear', 'mlp', 'neucf', 'fm', 'lstm', 'ease', 'itemknn'), \
            'Net type must be one of "linear", "mlp", "neu", "ease", "itemknn" or "lstm"'
        kw = dict(n_users=self.n_users, n_items=self.n_items, n_metadata=self.metadata_size,
                  n_factors=self.n_factors, use_metadata=self.use_metadata, use_cuda=self.use_cuda)
        if net_type == 'linear':
            print('Linear Collaborative Filtering')
            self.net = Linear(**kw)
        elif net_type == 'mlp':
            print('Multi Layer Perceptron')
            from .collaborative.mlp import MLP
            self.net = MLP(use_batch_norm=self.use_batch_norm, hidden_layers=self.hidden_layers,
                           use_bf16=self.use_amp, **kw)
        elif net_type == 'fm':
            print('Factorization Machine')
            self.net = FM(**kw)
        elif net_type == 'ease':
            print('Embarrassingly Shallow Autoencoder')
            if self.use_metadata:
                raise ValueError("net_type='ease' takes no metadata columns: the model is an item-item weight matrix "
                                 "over the interactions alone")
            from .collaborative.ease import EASE
            self.net = EASE(n_users=self.n_users, n_items=self.n_items)  # n_factors is ignored
            self.net.bind_history(self._seen_csr)
        elif net_type == 'itemknn':
            print('Item k-Nearest Neighbours')
            if self.use_metadata:
                raise ValueError("net_type='itemknn' takes no metadata columns: the model is item-item neighbour lists "
                                 "over the interactions alone")
            from .collaborative.itemknn import ItemKNN
            self.net = ItemKNN(n_users=self.n_users, n_items=self.n_items)  # n_factors is ignored
            self.net.bind_history(self._seen_csr)
        else:  # the reference silently leaves self.net undefined here (model.py:162-166)
            raise NotImplementedError(f'{net_type} is not implemented (nor is it in the reference)')
        # parameters are created on the host from torch's CPU generator (bit-identical init), then live in HBM
        if torch.cuda.is_available():
            self.net = self.net.to(_device())
            if tdist.world_info()[1] > 1:  # data parallel: every replica starts from rank 0's weights
                tdist.broadcast_([p.data for p in self.net.parameters()] + [b for b in self.net.buffers()])

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, net, batch):
        """Positive and negative scores of one batch (reference model.py:171-185), one fused kernel."""
        if hasattr(net, 'forward_pair'):
            return net.forward_pair(batch)
        positive = net.forward(batch, user_key='user_id', item_key='pos_item_id', metadata_key='pos_metadata_id')
        negative = net.forward(batch, user_key='user_id', item_key='neg_item_id', metadata_key='neg_metadata_id')
        return positive, negative

    def backward(self, loss_value, optimizer):
        """Generic autograd step (reference model.py:188-200) for callers that drive forward()/hinge_loss() themselves;
        fit() uses the fused engine instead."""
        optimizer.zero_grad()
        loss_value.backward()
        optimizer.step()
        return loss_value.item()

    # ------------------------------------------------------------------------------------------------ data staging
    def _id_dtype(self):
        big = max(self.n_users, self.n_items, *(list(self.metadata_size.values()) or [0]))
        return torch.int32 if big < 2 ** 31 else torch.int64

    def _host_epoch(self, data, loader):
        """All batches of one epoch in visiting order, consuming the reference's RNG streams exactly as its
        FastDataLoader would batch by batch (shuffle in __iter__, then the sampler walk in row order)."""
        order = loader.epoch_order()
        take = (lambda t: t[order]) if loader.shuffle else (lambda t: t)
        ep = {'user': take(data['user_id']), 'pos': take(data['pos_item_id'])}
        has_meta = 'pos_metadata_id' in data
        if has_meta:
            ep['pos_meta'] = take(data['pos_metadata_id'])
        if not self.dynamic_neg_sampling:
            ep['neg'] = take(data['neg_item_id'])
            if has_meta:
                ep['neg_meta'] = take(data['neg_metadata_id'])
        else:
            pos = ep['pos'].numpy()
            B = loader.batch_size
            neg = np.concatenate([sample_negatives_reference_stream(pos[i:i + B], self.n_items)
                                  for i in range(0, len(pos), B)]) if len(pos) else np.zeros(0, np.int64)
            ep['neg'] = torch.from_numpy(neg)
            if has_meta:
                ep['neg_meta'] = torch.from_numpy(self.data_processor.item_meta_table[neg])
        dt, dev = self._id_dtype(), _device()
        return {k: v.to(dt).contiguous().to(dev, non_blocking=True) for k, v in ep.items()}

    def _rank_rows(self, data):
        """This rank's rows of a split under data parallelism (the whole split in a single process).
        dp_partition 'user' (default): the rows whose user_id % world == rank — every user row then has exactly ONE
        writer, so the largest table never drifts between replicas and only item / metadata rows need the periodic
        average.  'contiguous': equal contiguous blocks.  pre_sharded: the caller's own cut — under
        dp_partition 'user' it is CHECKED to be the cut by user_id % world (one reduction per split, agreed over ranks so
        that every rank raises together): fit() never averages the user tables under that partition and its final
        gather_owned_rows_ takes rows r::world from rank r, so any other cut would silently replace trained user rows
        by another replica's stale ones.
        Rows are never dropped here: shards may differ in length.  Linear / FM steps contain no collective, so every
        rank simply runs its own number of steps; the MLP's lock-step (one gradient all-reduce per step) is kept by
        FitRunner, which runs the MINIMUM number of steps over ranks per epoch and leaves the shard whole — the rows
        beyond are a different set every epoch (the epoch shuffle), not a fixed tail.  evaluate() covers every row."""
        rank, world = tdist.world_info()
        if world == 1:
            return data
        key = id(data)
        cache = self._dev_cache.setdefault('shards', {})
        if key not in cache:
            if getattr(self, "pre_sharded", False):
                shard = data
                if getattr(self, "dp_partition", "user") == "user":
                    u = data['user_id']
                    ok = bool(((u % world) == rank).all()) if u.numel() else True
                    import torch.distributed as _d
                    dev = _device() if _d.get_backend() == 'nccl' else torch.device('cpu')
                    if tdist.allreduce_min_int(int(ok), dev) == 0:
                        raise ValueError(
                            "pre_sharded=True with dp_partition='user': every rank's interactions must satisfy "
                            f"user_id % world == rank (rank {rank}: {'ok' if ok else 'violated'}); pass "
                            "dp_partition='contiguous' for shards cut any other way (every table is then averaged)")
            elif getattr(self, "dp_partition", "user") == "user":
                keep = (data['user_id'] % world) == rank
                shard = {k: v[keep] for k, v in data.items()}
            else:
                s, e = tdist.equal_shard_bounds(data['user_id'].shape[0], rank, world)
                shard = {k: v[s:e] for k, v in data.items()}
            cache[key] = (data, shard)  # keeps `data` alive: its id() is the key
        return cache[key][1]

    def _device_stream(self, which):
        """The train/test interaction stream resident in HBM as int32 (rng='device')."""
        if which not in self._dev_cache:
            data = self._rank_rows(self.data_processor.train_data if which == 'train'
                                   else self.data_processor.test_data)
            dev = _device()
            d = {'user': data['user_id'].to(torch.int32).to(dev), 'pos': data['pos_item_id'].to(torch.int32).to(dev)}
            d['neg'] = data['neg_item_id'].to(torch.int32).to(dev) if 'neg_item_id' in data else None
            tab = self.data_processor.item_meta_table
            d['item_meta'] = None if tab is None else torch.from_numpy(tab).to(torch.int32).to(dev)
            self._dev_cache[which] = d
        return self._dev_cache[which]

    def _sampler(self):
        """ops.Sampler of the neg_sampling options, or None = the reference's sampler: uniform over the
        items other than the row's positive (dataset/dataset.py:435-447).  reject_seen uses the TRAIN split's (user, item)
        pairs; popularity the train split's item frequencies."""
        ns = getattr(self, "neg_sampling", None)
        if not ns:
            return None
        if 'sampler' not in self._dev_cache:
            st = self._device_stream('train')
            seen = self._seen_csr() if ns.get("reject_seen") else None
            self._dev_cache['sampler'] = ops.Sampler(k=ns.get("k", 1), popularity=ns.get("popularity", False), seen=seen,
                                                     stream_item=st['pos'], max_tries=ns.get("max_tries", 8),
                                                     mine=ns.get("mine"), candidates=ns.get("candidates", 8),
                                                     top=ns.get("top", 1))
        return self._dev_cache['sampler']

    def _eval_sampler(self):
        """evaluate(): the same candidate rules (reject_seen / popularity), every test row once, never mined (candidate 0
        of the same rules): loss and AUC stay comparable between mined and unmined runs."""
        sm = self._sampler()
        if sm is None or (sm.k == 1 and sm.mine is None):
            return sm
        if 'eval_sampler' not in self._dev_cache:
            ns = self.neg_sampling
            self._dev_cache['eval_sampler'] = ops.Sampler(k=1, popularity=ns.get("popularity", False), seen=sm.keep[0],
                                                          stream_item=sm.keep[1], max_tries=ns.get("max_tries", 8))
        return self._dev_cache['eval_sampler']

    def _seen_csr(self):
        """CSR of the train split's distinct (user, item) pairs (this rank's rows under data parallelism), built once:
        the sampler's reject_seen and recommend() / evaluate_ranking() exclude the same items."""
        if 'seen_csr' not in self._dev_cache:
            st = self._device_stream('train')
            self._dev_cache['seen_csr'] = ops.Sampler.seen_csr(st['user'], st['pos'], self.n_users, self.n_items)
        return self._dev_cache['seen_csr']

    def _item_meta_dev(self):
        tab = self.data_processor.item_meta_table
        if tab is None:
            return None
        if 'item_meta' not in self._dev_cache:
            self._dev_cache['item_meta'] = torch.from_numpy(tab).to(torch.int32).to(_device())
        return self._dev_cache['item_meta']

    _ITEM_ITEM = {'ease': ("a closed-form item-item model", "fit_ease", "EASE"),
                  'itemknn': ("an item-item neighbourhood model", "fit_itemknn", "item kNN")}

    def _refuse_ease(self, what, instead, exc=NotImplementedError):
        """net_type 'ease' / 'itemknn' have no embedding rows, no gradient steps and no pairwise loss: say what to call
        instead.  `instead` is worded for 'ease'; for 'itemknn' its fit_ease / EASE become fit_itemknn / item kNN."""
        if self.net_type in self._ITEM_ITEM:
            kind, fit, name = self._ITEM_ITEM[self.net_type]
            if self.net_type != 'ease':
                instead = instead.replace("fit_ease", fit).replace("EASE", name)
            raise exc(f"{what} does not apply to net_type={self.net_type!r} ({kind} without embedding "
                      f"rows): {instead}")

    def _make_trainer(self, optimizer, batch_size):
        self._refuse_ease("fit() / make_runner()", "call fit_ease()")
        if self.net_type == 'mlp':
            from .mlp_engine import MLPTrainer
            return MLPTrainer(self.net, optimizer, batch_size)
        return SparseScorerTrainer(self.net, optimizer, batch_size)

    # ------------------------------------------------------------------------------------------------ fit
    def make_runner(self, optimizer, batch_size):
        """The step-level driver fit() is built on (bench.py times exactly this object)."""
        return FitRunner(self, optimizer, batch_size)

    @_host_side
    def fit(self, optimizer, epochs=10, batch_size=512, profile_epochs: int = 0, sync_tables_every: int = 1,
            sync_bn: bool = False, loss: str = 'hinge', temperature: float = 1.0, logq_correction: bool = False,
            n_negatives: int = 1, margin: float = 1.0, rank_weight: str = 'log', l2=0.0):
        """Fits the model (reference model.py:203-288).  Per step: [shuffle slice + negative sampling] -> fused
        gather + scoring + hinge + backward -> sparse-row optimiser update; the loss stays on the device and is
        read back once per epoch (the reference syncs every step, model.py:200).

        Under torch.distributed (one process per GPU, RCCL over xGMI) every rank trains its shard of the training
        split with `batch_size` per rank and NO per-step collective on the embedding rows:
          * dp_partition 'user' (default): the stream is cut by user_id % world, so a user row is only ever written by
            its owner — user tables are never averaged; the owners' rows are all-gathered ONCE at the end of fit()
            (c4: 5.1 GB table, 0.64 GB sent per rank).  Item / metadata tables (and BatchNorm running statistics) are
            averaged every `sync_tables_every` epochs (0 = never): c4 = 516 MB per all-reduce, ~6 ms on one xGMI ring
            against an epoch of ~100 ms per rank;
          * dp_partition 'contiguous': every table is averaged at that cadence (c4: 5.6 GB, ~64 ms: use 'user');
          * MLP: the dense gradients are all-reduced every step, layer by layer while the backward is still running;
            sync_bn=True takes the train-mode BatchNorm statistics over the GLOBAL batch (two all-reduces of 2*H floats
            per layer and pass), so N ranks with batch B reproduce one process with batch N*B on the dense path.
        The printed loss is the mean over ranks.

        loss='softmax' (Linear and FM only): in-batch softmax over the batch's positives (Yi et al., RecSys 2019).  Row i
        scores its user against the positive item of every row j, z_ij / temperature - L_j, where L_j = log q of item
        p_j when logq_correction (q = the item's share of this rank's train rows, at least one count) and 0 otherwise;
        another row with the same item as row i is masked out; the row loss is logsumexp_j - the diagonal term, averaged
        over the batch.  The batches (and the negatives the loader draws, which the loss ignores) are those of a hinge
        run.  Under torch.distributed every rank's negatives are the positives of its OWN batch: nothing new crosses
        ranks.  evaluate() then reports this loss per test batch (AUC stays pairwise).  Not with neg_sampling options.

        neg_sampling={'mine': 'hardest', 'candidates': K, 'top': m} (constructor / from_tensors; Linear and FM, device RNG
        with dynamic negatives): score-aware hard-negative mining.  Per triple the sampler draws K candidates
        (1..64, default 8) under its usual rules (popularity / reject_seen / max_tries; candidate 0 is the negative an
        unmined run draws), one launch scores them under the current tables, and the step trains on one drawn uniformly
        among the m highest-scoring ones (1..K, default 1 = the hardest).  Hinge and BPR, every optimiser, metadata
        scorers and `k` visits per positive work unchanged; the steps run one by one (a mining launch, then the step),
        not on the slice-ahead presorted path, because the negative of step t depends on the tables after step t - 1.
        evaluate() keeps drawing unmined negatives, so its loss and AUC compare across mined and unmined runs.  Under
        torch.distributed every rank mines on its own replica with its own seed.

        n_negatives=K (1..64) and loss='sampled_softmax' (Linear and FM, rng='device' with dynamic_neg_sampling=True;
        DESIGN 4.8): every row trains on K sampled negatives.  Row i has user u, positive p and candidates c_0 .. c_{K-1}:
        c_j is the sampler's draw for the row's epoch position under seed s + j * 0xD1B54A32D192ED03 (mod 2^64), the
        candidate schedule of the mining option, so c_0 is the negative a plain run draws and popularity / reject_seen /
        max_tries / `k` visits per positive compose unchanged.  A candidate never equals the row's positive; candidates
        MAY repeat inside a row and every occurrence counts (sampling with replacement).
          loss='sampled_softmax' (any K >= 1): with z the scorer's value (Linear the score, FM the argument of its
            sigmoid, as retrieval, mining and the in-batch softmax use), zh_0 = z(u,p) / temperature and zh_{1+j} =
            z(u,c_j) / temperature, the row loss is logsumexp_s zh_s - zh_0, averaged over the batch.  logq_correction
            stays with loss='softmax': the popularity sampler's fallback draw makes its Q differ from the item frequency.
          loss in ('hinge', 'bpr') with K > 1: the row loss is the mean of the K pair losses (1/K) sum_j pair(s_p, s_cj)
            on the scores today's step uses (Linear the score, FM the sigmoid).  K = 1 is today's run, on today's paths.
        Every optimiser and metadata scorers work; the steps run one by one (one launch draws the ids, one kernel stages
        every gradient from the pre-update tables, then the per-table row updates).  Not with neg_sampling['mine'];
        K > 1 not with loss='softmax'.  evaluate() then reports the same loss on the test split with K candidates drawn by
        the evaluation sampler's rules; AUC stays pairwise on (p, c_0).  Under torch.distributed every rank draws and
        trains on its own replica: nothing new crosses ranks.

        loss='warp' with n_negatives=K (1..64), margin (> 0, default 1) and rank_weight ('log' | 'harmonic'; Linear and
        FM, rng='device' with dynamic_neg_sampling=True): WARP, the Weighted Approximate-Rank Pairwise loss of
        WSABIE (Weston et al. 2011), LightFM's default ranking loss.  The row's candidates c_0 .. c_{K-1} are those of
        n_negatives=K above (c_0 the negative a plain run draws; popularity / reject_seen / max_tries / `k` visits
        compose unchanged).  With z the scorer's value (Linear the score, FM the argument of its sigmoid, as sampled
        softmax, mining and retrieval use — on FM's sigmoid, whose values lie in (0, 1), a margin of 1 is always violated
        and WARP would degenerate to a constant weight), candidate j violates iff h_j = (z(u,c_j) - z(u,p)) + margin > 0.
        The row trains on the FIRST violator c_J alone: its loss is w_J * h_J, 0 when no candidate violates.  w_J is the
        rank estimate from the J + 1 draws it took: with r = floor((n_items - 1) / (J + 1)), 'log' gives log(max(1, r))
        (LightFM's form), 'harmonic' sum_{i=1..r} 1 / i (Weston's); no clipping.  n_items - 1 is used whatever the
        sampler's options are: popularity or seen rejection make the estimate approximate.  Badly ranked rows take large
        steps, rows already ranked well none.  Every optimiser and metadata scorers work; the steps run one by one (one
        launch draws the ids, one kernel finds the violators and stages the gradients of (user, positive, c_J), then
        today's row updates).  Not with neg_sampling['mine'], temperature or logq_correction; margin and rank_weight
        belong to loss='warp' alone.  evaluate() then reports the WARP loss over K candidates drawn by the evaluation
        sampler's rules; AUC stays pairwise on (p, c_0).  Under torch.distributed nothing new crosses ranks.

        l2=lambda (Linear and FM): per-sample L2 regularisation of the embedding rows a batch touches —
        LightFM's user_alpha / item_alpha, the lambda of the BPR paper.  A non-negative finite number, or a mapping with
        keys among 'user', 'item', 'metadata' (missing keys mean 0); a 1-wide table (bias / linear term) takes its
        group's coefficient.  Per batch of B rows the step minimises
          (1/B) sum_b [ loss_b + 1/2 sum_{references r of row b} lambda_group(r) (|W_r|^2 + w_r^2) ]
        where the references of row b are the rows its gradients are staged for: its user, its item slots (the pair, the
        positive alone under loss='softmax', the positive and all K candidates under n_negatives=K, (positive, chosen
        candidate) under loss='warp' — c_0 for a row without a violator: the penalty belongs to the reference, not to
        the violation) and the metadata rows of those slots.  So every staged reference's gradient gains lambda_group / B
        times its PRE-update row (as loss.backward() before optimizer.step() reads it); a row referenced c times in the
        batch receives the term c times; 1/B is that of the actual batch, the partial last one included; a row no id of
        the batch references is left bit-identical.  The penalised gradient goes through the optimiser's rule unchanged
        (torch's coupled weight_decay semantics, restricted to touched rows).  Combines with every loss, n_negatives,
        neg_sampling option (mining included), rng and optimiser.  With any coefficient non-zero the steps run one by
        one on the staged per-step loop (as n_negatives > 1 does), with one more launch per step; all coefficients zero
        is today's run on today's paths, bit for bit.  The printed training loss stays the data loss without the
        penalty and evaluate() is unchanged, so runs with and without l2 compare.  Under torch.distributed nothing new
        crosses ranks.  net_type='mlp': ValueError for any non-zero coefficient."""
        # loss: 'hinge' = the reference's only loss (helper/loss.py:5-9, model.py:282); 'bpr' = -log sigmoid(pos - neg),
        # the alternative BASELINE.json's north_star names (evaluate() then reports that loss too); 'softmax' = the
        # in-batch softmax (engine.SparseScorerTrainer.softmax_step; not a pair loss, so not in LOSS_ID)
        self._refuse_ease("fit()", "call fit_ease(), which needs no optimiser")
        from ._lib import LOSS_ID, LOSS_SAMPLED_SOFTMAX
        if loss not in LOSS_ID and loss not in ('softmax', 'sampled_softmax', 'warp'):
            raise ValueError(f"loss must be one of {sorted(list(LOSS_ID) + ['softmax', 'sampled_softmax', 'warp'])}")
        if isinstance(n_negatives, bool) or not isinstance(n_negatives, (int, np.integer)) or not 1 <= n_negatives <= 64:
            raise ValueError(f"n_negatives must be an integer in 1..64, got {n_negatives!r}")
        n_negatives = int(n_negatives)
        l2 = _check_l2(l2, self.net_type)
        multineg = loss == 'sampled_softmax' or n_negatives > 1
        if loss == 'softmax' and n_negatives > 1:
            raise ValueError("n_negatives > 1 does not combine with loss='softmax' (its negatives are the batch's other "
                             "positives); loss='sampled_softmax' is the softmax over sampled negatives")
        warp = loss == 'warp'
        if warp:
            multineg = False  # (the same candidates, its own kernel and step: engine.SparseScorerTrainer.warp_step)
            try:
                margin = float(margin)
            except (TypeError, ValueError):
                raise ValueError(f"margin must be a positive finite number, got {margin!r}") from None
            if not (math.isfinite(margin) and margin > 0):
                raise ValueError(f"margin must be a positive finite number, got {margin!r}")
            if rank_weight not in ('log', 'harmonic'):
                raise ValueError(f"rank_weight must be 'log' or 'harmonic', got {rank_weight!r}")
        elif margin != 1.0 or rank_weight != 'log':
            raise ValueError("margin and rank_weight apply to loss='warp' only")
        if multineg or warp:
            what = ("loss='warp'" if warp else
                    "loss='sampled_softmax'" if loss == 'sampled_softmax' else f"n_negatives={n_negatives}")
            if self.net_type not in ('linear', 'fm'):
                raise ValueError(f"{what} trains the Linear and FM scorers (net_type 'linear' or 'fm'), not "
                                 f"net_type={self.net_type!r}")
            if self.rng != 'device':
                raise ValueError(f"{what} draws its negatives with the device sampler: it needs rng='device', not "
                                 f"rng={self.rng!r}")
            if not self.dynamic_neg_sampling:
                raise ValueError(f"{what} needs dynamic_neg_sampling=True (there is one static negative per row)")
            if (getattr(self, 'neg_sampling', None) or {}).get('mine') is not None:
                if warp:
                    raise ValueError(f"{what} trains on the first violator among its candidates: it does not combine "
                                     "with neg_sampling['mine'] (which picks by score)")
                raise ValueError(f"{what} trains on every candidate: it does not combine with neg_sampling['mine'] "
                                 "(which trains on one of them)")
            if logq_correction:
                raise ValueError("logq_correction applies to loss='softmax' only (the popularity sampler's fallback draw "
                                 "makes the sampled candidates' Q differ from the item frequency)")
        if loss == 'softmax':
            if self.net_type not in ('linear', 'fm'):
                raise ValueError("loss='softmax' trains the Linear and FM scorers (net_type 'linear' or 'fm'), "
                                 f"not net_type={self.net_type!r}")
            if getattr(self, 'neg_sampling', None):
                raise ValueError("loss='softmax' takes its negatives from the batch: it does not combine with "
                                 "neg_sampling options (k > 1 would repeat positives inside a batch)")
        if loss in ('softmax', 'sampled_softmax'):
            try:
                tau = float(temperature)
            except (TypeError, ValueError):
                raise ValueError(f"temperature must be a positive finite number, got {temperature!r}") from None
            if not (math.isfinite(tau) and tau > 0):
                raise ValueError(f"temperature must be a positive finite number, got {temperature!r}")
        elif temperature != 1.0 or logq_correction:
            raise ValueError("temperature applies to loss='softmax' / 'sampled_softmax' and logq_correction to "
                             "loss='softmax' only")
        if self.net_type == 'mlp':
            self.net.compute.sync_bn = bool(sync_bn)
        runner = self.make_runner(optimizer, batch_size)
        obj = self._objective = Objective(
            kind='softmax' if loss == 'softmax' else 'multineg' if multineg else 'warp' if warp else 'pair',
            loss_id=LOSS_ID.get(loss, LOSS_SAMPLED_SOFTMAX if multineg else 0), K=n_negatives,
            temperature=tau if loss in ('softmax', 'sampled_softmax') else 1.0,
            logq=self._logq(runner.data) if loss == 'softmax' and logq_correction else None,
            margin=margin, rank_weight=rank_weight)
        if obj.kind == 'softmax':  # engine.SparseScorerTrainer.softmax_step
            runner.trainer.softmax = (obj.temperature, obj.logq)
        elif obj.kind == 'multineg':  # K sampled negatives per positive: engine.SparseScorerTrainer.multineg_step
            runner.trainer.multineg = (obj.K, obj.loss_id, obj.temperature)
        elif obj.kind == 'warp':  # the first margin violator among K candidates: engine.SparseScorerTrainer.warp_step
            runner.trainer.warp = (obj.K, obj.margin, ops.warp_rank_weights(self.n_items, obj.K, obj.rank_weight, _device()))
        else:
            runner.trainer.loss_id = obj.loss_id
        if l2 is not None:  # engine.SparseScorerTrainer._add_l2: one launch between a step's staging and its row updates
            runner.trainer.l2 = l2
        self.loss = loss
        for epoch in range(epochs):
            self.net = self.net.train()
            prof = None
            if profile_epochs > 0 and epoch == 0:
                print(f"\n--- Starting Profiling for Epoch {epoch+1} ---")
                prof = torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU,
                                                          torch.profiler.ProfilerActivity.CUDA],
                                              record_shapes=True, profile_memory=True, with_stack=True)
                prof.__enter__()
            runner.more_epochs = epoch < epochs - 1  # lets the last slice's steps hide the next epoch's first presort
            runner.begin_epoch()
            runner.run_steps(runner.num_batches)
            if runner.more_epochs:
                runner.prepare_next_epoch()  # host work of epoch e+1 while the GPU runs epoch e
            avg_loss = runner.end_epoch()
            world = tdist.world_info()[1]
            if world > 1:
                avg_loss = tdist.allreduce_scalar_sum([avg_loss], _device())[0] / world
                if sync_tables_every and (epoch + 1) % sync_tables_every == 0:
                    self._sync_replicas()
            if prof is not None:
                prof.__exit__(None, None, None)
                print("--- Profiler Results (First Epoch) ---")
                print(prof.key_averages().table(sort_by="self_cpu_time_total", row_limit=20))
            print(f'|--- Epoch {epoch+1}/{epochs} --- Training Loss: {avg_loss:.4f}')
        if tdist.world_info()[1] > 1 and self.dp_partition == 'user':
            for t in self._user_tables():  # every replica gets the owners' user rows
                tdist.gather_owned_rows_(t.data)

    def _logq(self, data):
        """(n_items,) fp32 log q on the device: q = max(count of the item in `data`'s rows, 1) / number of rows."""
        dev = _device()
        pos = data['pos_item_id'].to(dev).long()
        counts = torch.bincount(pos, minlength=self.n_items).clamp_min(1).double()
        return torch.log(counts / max(pos.numel(), 1)).float().contiguous()

    def _user_tables(self):
        """Tables indexed by user id (Linear / FM: the embedding and the 1-wide term; MLP: the embedding)."""
        if hasattr(self.net, 'embedding_params'):
            return [self.net.embedding_params()[0]]
        ps = self.net.table_params()
        return [ps[0], ps[2]]

    def _sync_replicas(self):
        """Periodic re-synchronisation of the replicas: the mean over ranks of every embedding table that has more than
        one writer (all but the user tables under dp_partition 'user') and of the BatchNorm running statistics."""
        emb = self.net.embedding_params() if hasattr(self.net, 'embedding_params') else self.net.table_params()
        if self.dp_partition == 'user':
            owned = {id(p) for p in self._user_tables()}
            emb = [p for p in emb if id(p) not in owned]
        bufs = [b for b in self.net.buffers() if b.is_floating_point()]
        tdist.average_tables_([p.data for p in emb] + bufs)

    # ------------------------------------------------------------------------------------------------ ALS
    def _check_fit_als(self, iterations, regularization, alpha, cg_steps):
        """Argument checks of fit_als (before any device work)."""
        self._refuse_ease("fit_als()", "call fit_ease()", ValueError)
        if self.net_type not in ('linear', 'fm'):
            raise ValueError(f"fit_als needs net_type 'linear' or 'fm': with net_type={self.net_type!r} (mlp) a score "
                             "is not the inner product of a user row and an item row")
        if self.use_metadata:
            raise ValueError("fit_als takes a model without metadata columns: with metadata an item is its row plus its "
                             "metadata rows, and the alternating solves are no longer independent per row")
        if self.n_factors > ops._lib.RETRIEVE_DMAX:
            raise ValueError(f"fit_als takes n_factors <= {ops._lib.RETRIEVE_DMAX} (TRS_RETRIEVE_DMAX), got "
                             f"{self.n_factors}")
        if tdist.world_info()[1] > 1:
            raise NotImplementedError("fit_als runs in a single process: under torch.distributed (world > 1) every rank "
                                      "holds a shard of the interactions, and a row's solve needs all of its pairs")

        def integer(v, name, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")

        def number(v, name, positive):
            ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)
            f = float(np.float32(v)) if ok and abs(v) <= 3.4e38 else float("nan")  # the kernel takes it as fp32
            if not (f > 0 if positive else f >= 0):
                raise ValueError(f"{name} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
        integer(iterations, "iterations", 1, 1 << 20)
        integer(cg_steps, "cg_steps", 1, 256)
        number(regularization, "regularization", True)
        number(alpha, "alpha", False)

    def _als_csrs(self):
        """(user -> sorted items, item -> sorted users) CSRs of the train split's distinct pairs, built once."""
        seen = self._seen_csr()
        if 'seen_csr_items' not in self._dev_cache:
            st = self._device_stream('train')
            self._dev_cache['seen_csr_items'] = ops.Sampler.seen_csr(st['pos'], st['user'], self.n_items, self.n_users)
        return seen, self._dev_cache['seen_csr_items']

    def _als_loss(self, X, Y, GX, GY, pairs, lam, alpha):
        """The ALS objective (fit_als docstring) as a Python float: the Gram term and the norms from the fp32 Gram
        matrices, the observed term from one fp32 scoring pass over the train pairs (1-wide tables are zero: the Linear
        score is <x_u, y_i>), everything summed in float64."""
        dev = X.device
        users, items = pairs
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        Bt, keep = ops.make_batch(users, items, None, None, None, err)
        s, _ = ops.score_forward('linear', self.net.tables(), Bt, users.numel(), dev, want_neg=False)
        check_err_flag(err, "fit_als")
        s = s.double()
        observed = ((1.0 + alpha) * (1.0 - s) ** 2 - s ** 2).sum()
        gx, gy = GX.double(), GY.double()
        return float((gx * gy).sum() + observed + lam * (torch.diagonal(gx).sum() + torch.diagonal(gy).sum()))

    @_host_side
    def fit_als(self, iterations: int = 15, regularization: float = 0.1, alpha: float = 10.0, cg_steps: int = 3,
                return_loss: bool = False):
        """Implicit-feedback weighted alternating least squares (Hu, Koren, Volinsky 2008; the main model of the
        `implicit` package) on the train split's distinct (user, item) pairs: preference 1 with confidence 1 + alpha on
        those pairs, preference 0 with confidence 1 everywhere else, L2 coefficient `regularization` on both tables.  No
        learning rate, no negative sampler; deterministic.

        One iteration is the user half-sweep, then the item half-sweep.  A half-sweep is two launches: the Gram matrix
        of the frozen table (trs_als_gram), then every row of the other table takes at most cg_steps conjugate-gradient
        steps from its current value (trs_als_solve; the exact rule is in include/trs.h "implicit ALS").  A row without
        a pair becomes 0.  The sweeps start from the model's current user / item tables — the seeded init, or what fit()
        left — so fit_als(1) called five times equals fit_als(5) bit for bit.

        Writes the two n_factors-wide tables in place and zeroes the 1-wide tables (user_bias / item_bias, or FM's
        linear_user / linear_item) before the first sweep: the Linear score and FM's logit are then both <x_u, y_i>, and
        recommend(), rank_items(), similar_items(), recommend_diverse(), evaluate_ranking() and the fold-in calls rank
        by the ALS score.  Optimiser state is not touched; nothing derived from the tables is cached across calls.

        return_loss: a float64 CPU tensor of iterations + 1 values of
            L = sum_u x_u^T G_Y x_u + sum_{(u,i) observed} [(1 + alpha)(1 - s_ui)^2 - s_ui^2] + lambda (|X|^2 + |Y|^2),
        s = <x_u, y_i>, G_Y = Y^T Y, the first taken before the first sweep (after the 1-wide tables are zeroed).  The
        first term is the Frobenius product of the two Gram matrices; the observed term comes from one scoring pass
        over the train pairs; sums in float64.  Without return_loss none of this runs.

        net_type 'linear' or 'fm' without metadata columns, n_factors <= TRS_RETRIEVE_DMAX, single process: ValueError /
        NotImplementedError otherwise, before any device work."""
        self._check_fit_als(iterations, regularization, alpha, cg_steps)
        iterations, cg_steps = int(iterations), int(cg_steps)
        lam, alpha = float(regularization), float(alpha)
        dev = _device()
        ps = self.net.table_params()
        X, Y = ps[0].data, ps[1].data
        by_user, by_item = self._als_csrs()
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.no_grad():
            ps[2].data.zero_()
            ps[3].data.zero_()
            losses = []
            if return_loss:
                off, items = by_user
                pairs = (torch.repeat_interleave(torch.arange(self.n_users, dtype=torch.int32, device=dev),
                                                 off[1:] - off[:-1]), items)
                GX = ops.als_gram(X)
            for _ in range(iterations):
                GY = ops.als_gram(Y)
                if return_loss:
                    losses.append(self._als_loss(X, Y, GX, GY, pairs, lam, alpha))
                ops.als_solve(Y, GY, by_user, lam, alpha, cg_steps, X, err)
                GX = ops.als_gram(X)
                ops.als_solve(X, GX, by_item, lam, alpha, cg_steps, Y, err)
            if return_loss:
                losses.append(self._als_loss(X, Y, GX, ops.als_gram(Y), pairs, lam, alpha))
        check_err_flag(err, "fit_als")
        return torch.tensor(losses, dtype=torch.float64) if return_loss else None

    # ------------------------------------------------------------------------------------------------ LightGCN
    def _check_fit_lightgcn(self, epochs, lr, batch_size, layers, optimizer, loss, l2, seed, max_tries):
        """Argument checks of fit_lightgcn (before any device work)."""
        what = "fit_lightgcn"
        self._refuse_ease("fit_lightgcn()", "call fit_ease()", ValueError)
        if self.net_type not in ('linear', 'fm'):
            raise ValueError(f"{what} needs net_type 'linear' or 'fm': with net_type={self.net_type!r} (mlp) a score is "
                             "not the inner product of a user row and an item row")
        if self.use_metadata:
            raise ValueError(f"{what} takes a model without metadata columns: the graph it propagates over has user and "
                             "item nodes only")
        if self.n_factors > ops._lib.RETRIEVE_DMAX:
            raise ValueError(f"{what} takes n_factors <= {ops._lib.RETRIEVE_DMAX} (TRS_RETRIEVE_DMAX), got "
                             f"{self.n_factors}")
        if tdist.world_info()[1] > 1:
            raise NotImplementedError(f"{what} runs in a single process: under torch.distributed (world > 1) every rank "
                                      "holds a shard of the interactions, and a row's propagation needs all of its pairs")

        def integer(v, name, lo, hi=None):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
                raise ValueError(f"{what}: {name} must be an integer in {lo}..{'' if hi is None else hi}, got {v!r}")

        def number(v, name, positive):
            ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)
            f = float(np.float32(v)) if ok and abs(v) <= 3.4e38 else float("nan")  # the kernels take it as fp32
            if not (f > 0 if positive else f >= 0):
                raise ValueError(f"{what}: {name} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
        integer(epochs, "epochs", 1)
        integer(batch_size, "batch_size", 1)
        integer(layers, "layers", 0, ops._lib.LGCN_LAYERS_MAX)
        integer(seed, "seed", 0)
        integer(max_tries, "max_tries", 1, 1 << 20)
        number(lr, "lr", True)
        number(l2, "l2", False)
        if optimizer not in ('adam', 'sgd'):
            raise ValueError(f"{what}: optimizer must be 'adam' or 'sgd', got {optimizer!r}")
        if loss not in ('bpr', 'hinge'):
            raise ValueError(f"{what}: loss must be 'bpr' or 'hinge', got {loss!r}")
        if self.n_items < 2:
            raise ValueError(f"{what}: sampling a negative needs n_items >= 2")

    @_host_side
    def fit_lightgcn(self, epochs: int = 10, lr: float = 1e-3, batch_size: int = 16384, layers: int = 3,
                     optimizer: str = 'adam', loss: str = 'bpr', l2: float = 1e-4, seed: int = 0,
                     reject_seen: bool = True, max_tries: int = 8, restart: bool = False, return_loss: bool = False):
        """LightGCN (He et al., SIGIR 2020) on the graph of the train split's distinct (user, item) pairs.  With A^ the
        symmetric normalised adjacency (A^[u][i] = 1 / sqrt(deg_u deg_i) on a pair) and E0 = [U0; V0] the base tables,
            Final = 1/(layers + 1) * sum_{k = 0..layers} A^^k E0,        score(u, i) = <Final_u, Final_i>;
        no weights beyond the two tables.  The sum is evaluated in Horner form (F_K = E0, F_k = E0 + A^ F_{k+1}), the
        gradient is the same recurrence on dL/dFinal; every hop is one launch of trs_lgcn_propagate per side (the exact
        rule is in include/trs.h "LightGCN").  layers = 0 is plain matrix factorisation with the pairwise loss.

        Every epoch visits every train row once, in a permutation seeded by (seed, epoch); the last partial batch runs.
        One step = one negative per row from the device sampler (uniform over the items other than the row's positive;
        with reject_seen an item the user has a train pair with is redrawn, at most max_tries candidates), the forward,
        the 'bpr' or 'hinge' loss on (score of the positive, score of the negative), the backward, and the update of
        the base tables: optimizer 'sgd' is plain SGD at `lr`; 'adam' is torch.optim.Adam's rule at its default betas
        and eps on every element of both tables (LightGCN's gradient is dense).  l2: l2 / B times the pre-update base
        row is added to the gradient of every reference (user, positive, negative) of a batch of B rows, as fit(l2=)
        means it.  No optimiser object, no host sync inside an epoch.

        The base tables and the layer count become buffers of the net (lgcn_user_base, lgcn_item_base, lgcn_layers;
        state_dict() carries them).  The net's user / item tables are left holding Final and its 1-wide tables are
        zeroed, so recommend(), rank_items(), similar_items(), recommend_diverse(), evaluate_ranking(),
        evaluate_ranks(), evaluate() and the fold-in calls answer from the LightGCN score.
        A later call continues from the base tables when `layers` is the same, restart is false and the tables still
        equal the forward of the buffers bit for bit (the check costs one forward; the operator is deterministic, so a
        fit() or fit_als() in between is seen).  Otherwise the current tables become the new base.  Adam's moments do
        NOT survive a call: every call starts them from zero.  The count of epochs done, which keys the permutations
        and the sampler, stays with this model object: a model restored from a state_dict() continues from the
        restored tables but draws the permutations and negatives of epochs 0, 1, ... again.
        The buffers are a second pair of tables.  A later fit() or fit_als() leaves them in the net and in
        state_dict() (the next fit_lightgcn() re-bases over them); to drop them set net.lgcn_user_base,
        net.lgcn_item_base and net.lgcn_layers to None.

        Memory: besides the net's tables a call holds buffers of the size of both tables together — 4 of them with
        'sgd' (the base tables, the dense gradient, the work tables of the recurrence), 6 with 'adam' (the two moments
        on top); it raises RuntimeError when the device has less free memory than that.
        Returns None, or with return_loss the (epochs,) float64 mean row loss of every epoch.
        Before any device work: ValueError for another net_type, metadata columns, n_factors > TRS_RETRIEVE_DMAX, layers
        outside 0..8, n_items < 2 or a bad argument; NotImplementedError under torch.distributed with more than one
        rank."""
        what = "fit_lightgcn"
        self._check_fit_lightgcn(epochs, lr, batch_size, layers, optimizer, loss, l2, seed, max_tries)
        epochs, batch_size, layers, seed, max_tries = int(epochs), int(batch_size), int(layers), int(seed), int(max_tries)
        lr, l2 = float(lr), float(l2)
        from .engine import LightGCNTrainer
        dev = _device()
        net = self.net = self.net.train()
        ps = net.table_params()
        U, V = ps[0].data, ps[1].data
        have = net.lgcn_user_base is not None and net.lgcn_item_base is not None and net.lgcn_layers is not None
        pair_bytes = 4 * (self.n_users + self.n_items) * int(self.n_factors)
        need = (LightGCNTrainer.BUFFERS[optimizer] - (1 if have else 0)) * pair_bytes
        free = torch.cuda.mem_get_info(dev)[0]
        if free < need:
            raise RuntimeError(f"{what}: optimizer={optimizer!r} needs {LightGCNTrainer.BUFFERS[optimizer]} buffers of "
                               f"the size of both tables ({pair_bytes} bytes each); the device has {free} bytes free")
        graph = self._als_csrs()
        st = self._device_stream('train')
        n = int(st['user'].numel())
        with torch.no_grad():
            ps[2].data.zero_()
            ps[3].data.zero_()
            resume = have and not restart and int(net.lgcn_layers.item()) == layers
            if not have:
                net.lgcn_user_base, net.lgcn_item_base = U.clone(), V.clone()
                net.lgcn_layers = torch.tensor([layers], dtype=torch.int64, device=dev)
            trainer = LightGCNTrainer(net, (net.lgcn_user_base, net.lgcn_item_base), graph, layers,
                                      max(min(batch_size, n), 1), lr, ops._lib.LOSS_ID[loss], optimizer, l2)
            if resume:  # do the tables still hold the forward of the buffers?
                keep_u, keep_v = U.clone(), V.clone()
                trainer.forward()
                resume = torch.equal(U, keep_u) and torch.equal(V, keep_v)
                if not resume:
                    U.copy_(keep_u)
                    V.copy_(keep_v)
                del keep_u, keep_v
            if not resume:  # the current tables are the new base
                net.lgcn_user_base.copy_(U)
                net.lgcn_item_base.copy_(V)
                net.lgcn_layers.fill_(layers)
                trainer.forward()
                self._lgcn_epochs_done = 0
            loss_sums = torch.zeros(epochs, dtype=torch.float32, device=dev)
            if n:
                B = min(batch_size, n)
                sampler = ops.Sampler(seen=self._seen_csr() if reject_seen else None, max_tries=max_tries)
                done = getattr(self, "_lgcn_epochs_done", 0)
                for ep in range(epochs):
                    shuffle_key = _mix64(seed, done + ep)
                    sample_seed = _mix64(seed ^ 0x16C7, done + ep)
                    for s in range(0, n, B):
                        ids = ops.batch_prepare(st['user'], st['pos'], None, shuffle_key, s, min(B, n - s), self.n_items,
                                                sample_seed, s, sampler=sampler)
                        trainer.lgcn_step(ids['user'], ids['pos'], ids['neg'], loss_sums[ep:ep + 1])
                    avg = float(loss_sums[ep].item()) / n  # the epoch's one read
                    print(f'|--- Epoch {ep+1}/{epochs} --- Training Loss: {avg:.4f}')
                self._lgcn_epochs_done = done + epochs
            trainer.check_errors()
        return (loss_sums.cpu().to(torch.float64) / max(n, 1)) if return_loss else None

    # ------------------------------------------------------------------------------------------------ EASE
    @_host_side
    def fit_ease(self, regularization: float = 0.5):
        """Closed-form EASE (Steck 2019; reference collaborative/ease.py) on the train split's distinct (user, item)
        pairs X:  P = (X^T X + regularization I)^-1,  B[i][j] = -P[i][j] / P[j][j],  B[i][i] = 0;  a user's scores are
        the sum of the B rows of the user's train items.  No learning rate, no sampler, deterministic: two calls give
        the same B bit for bit.  regularization defaults to the reference's lambda_ = 0.5, which suits toy data; real
        data usually wants hundreds (Steck reports 500 for ML-20M, 1000 for Netflix).
        X is binary: a pair that occurs several times counts once (Steck's definition; the reference's sparse matrix adds
        repeats up, and agrees on data without them).
        Device work: trs_ease_gram (fp64 atomics of exact integer counts), trs_ease_invert (blocked Cholesky, triangular
        inverse and product on the fp64 matrix cores), trs_ease_weights (fp32 B); the rule is in include/trs.h "EASE".
        Memory: two fp64 matrices and the fp32 B, 20 bytes per entry of the catalogue squared (padded to a multiple of
        64) — 5.4 GB at 16 384 items, 21.5 GB at TRS_EASE_NMAX = 32 768; the fp64 matrices are freed on return and B
        (4 n_items^2 bytes) stays as a buffer of the net, in state_dict().
        Afterwards predict(), predict_many(), recommend(), rank_items(), evaluate_ranking(), evaluate_ranks(),
        recommend_for_histories() and item_weights() answer from B.
        Before any device work: ValueError for another net_type, a regularization that is not a finite number > 0 or
        n_items > TRS_EASE_NMAX; NotImplementedError under torch.distributed with more than one rank (the seen CSR is
        this rank's shard); RuntimeError when the device reports less free memory than the 20 bytes per entry."""
        if self.net_type != 'ease':
            raise ValueError(f"fit_ease needs net_type='ease', not {self.net_type!r}: call fit() or fit_als()")
        lam = regularization
        ok = isinstance(lam, (int, float, np.integer, np.floating)) and not isinstance(lam, bool) and math.isfinite(lam)
        if not ok or not lam > 0:
            raise ValueError(f"regularization must be a finite number > 0, got {regularization!r}")
        nmax = ops._lib.EASE_NMAX
        if self.n_items > nmax:
            raise ValueError(f"fit_ease takes n_items <= {nmax} (TRS_EASE_NMAX), got {self.n_items}: the dense weight "
                             f"matrix and the two fp64 work matrices need 20 * n_items^2 bytes of device memory, "
                             f"{20 * self.n_items ** 2 / 1e9:.1f} GB here")
        if tdist.world_info()[1] > 1:
            raise NotImplementedError("fit_ease runs in a single process: under torch.distributed (world > 1) the seen "
                                      "CSR is this rank's shard of the interactions, and X^T X needs all of them")
        _device()
        nbar = ops.ease_padded(self.n_items)
        need = 20 * nbar * nbar
        free = int(torch.cuda.mem_get_info()[0])
        if free < need:
            raise RuntimeError(f"fit_ease needs {need / 1e9:.2f} GB of free device memory for {self.n_items} items (two "
                               f"fp64 matrices and the fp32 weights), the device reports {free / 1e9:.2f} GB free")
        seen = self._seen_csr()
        err = torch.zeros(2, dtype=torch.int32, device=seen[0].device)
        A = ops.ease_gram(seen, self.n_items, float(lam), err[0:1])
        ops.ease_invert(A, err[1:2])
        B = ops.ease_weights(A, self.n_items)
        del A
        check_err_flag(err[0:1], "fit_ease")
        if int(err[1].item()):
            raise RuntimeError("fit_ease: X^T X + regularization I is not numerically positive definite (a pivot of the "
                               "Cholesky factorisation was not positive and finite); raise regularization")
        self.net.set_weights(B, seen)

    # ------------------------------------------------------------------------------------------------ item kNN
    @_host_side
    def fit_itemknn(self, neighbours: int = 100, similarity: str = 'cosine', shrinkage: float = 0.0):
        """Sparse item-kNN on the train split's distinct (user, item) pairs: c(i, j) = the users who hold both items,
        similarity 'cosine' c / (sqrt(n_i n_j) + h), 'jaccard' c / (n_i + n_j - c + h), 'conditional' c / (n_i + h) or
        'count' c, with h = shrinkage; every item keeps its `neighbours` most similar items (ties by ascending item
        row), and a user's scores are the sums over the neighbour lists of the user's train items.  The lists are pruned
        per row: item i votes for its own nearest items.  No learning rate, no sampler; the counts are integers and the
        similarity is formed in fp64 and rounded to fp32 once, so two calls give the same lists bit for bit (the rule is
        in include/trs.h "item kNN").
        Device work: one launch of trs_knn_build over the two CSRs of the train pairs; nothing of size n_items^2 is
        allocated, the model is 8 * n_items * neighbours bytes (buffers of the net, in state_dict()).
        Afterwards predict(), predict_many(), recommend(), rank_items(), evaluate_ranking(), evaluate_ranks(),
        recommend_for_histories() and item_weights() answer from the lists.
        Before any device work: ValueError for another net_type, an unknown similarity, neighbours outside
        1..TRS_KNN_KMAX or a shrinkage that is not a finite number >= 0; NotImplementedError under torch.distributed
        with more than one rank (the CSRs are this rank's shard)."""
        if self.net_type != 'itemknn':
            raise ValueError(f"fit_itemknn needs net_type='itemknn', not {self.net_type!r}: call fit(), fit_als() or "
                             f"fit_ease()")
        kinds = ops._lib.KNN_KIND
        if not isinstance(similarity, str) or similarity not in kinds:
            raise ValueError(f"similarity must be one of {sorted(kinds)}, got {similarity!r}")
        kmax = ops._lib.KNN_KMAX
        if isinstance(neighbours, bool) or not isinstance(neighbours, (int, np.integer)) or \
                not 1 <= int(neighbours) <= kmax:
            raise ValueError(f"neighbours must be an integer in 1..{kmax} (TRS_KNN_KMAX), got {neighbours!r}")
        h = shrinkage
        ok = isinstance(h, (int, float, np.integer, np.floating)) and not isinstance(h, bool) and math.isfinite(h)
        if not ok or not h >= 0:
            raise ValueError(f"shrinkage must be a finite number >= 0, got {shrinkage!r}")
        if tdist.world_info()[1] > 1:
            raise NotImplementedError("fit_itemknn runs in a single process: under torch.distributed (world > 1) the "
                                      "CSRs are this rank's shard of the interactions, and a co-occurrence count needs "
                                      "all of them")
        _device()
        by_user, by_item = self._als_csrs()
        err = torch.zeros(1, dtype=torch.int32, device=by_user[0].device)
        ids, w = ops.knn_build(by_user, by_item, self.n_items, similarity, float(h), int(neighbours), err)
        check_err_flag(err, "fit_itemknn")
        self.net.set_neighbours(ids, w, by_user, kinds[similarity], float(h))

    def _item_item_recommend_for_histories(self, score_csr_rows, dev, histories, top_k, exclude_seen, return_scores):
        """recommend_for_histories on an item-item model (EASE, item kNN): score rows of the histories' own CSR
        (score_csr_rows(hist, rows) -> (len(rows), n_items) fp32 on `dev`), mask, top-k, ids back."""
        off, items, rank = self._history_csr(histories)
        n = rank.size
        k = min(int(top_k), self.n_items)
        if k <= 0 or n == 0:
            return self._empty_topk(n, k, return_scores)
        dev = dev()
        hist = (torch.from_numpy(off).to(dev), torch.from_numpy(items).to(dev))
        mask = bool(exclude_seen) and items.size > 0  # every history empty: nothing to exclude
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        for s in range(0, n, self.GENERIC_CHUNK):
            us = torch.arange(s, min(s + self.GENERIC_CHUNK, n), dtype=torch.int64, device=dev)
            rows = score_csr_rows(hist, us)
            if mask:
                ops.mask_seen(rows, us, hist)
                n_seen = hist[0][us + 1] - hist[0][us]
            else:
                n_seen = torch.zeros_like(us)
            ids[s:s + us.numel()], scores[s:s + us.numel()] = self._topk_rows(rows, rows, k, self.n_items - n_seen)
        r = torch.from_numpy(rank)
        ids = self._original_ids(ids.cpu()[r], getattr(self.data_processor, "item_index", None))
        return (ids, scores.cpu()[r]) if return_scores else ids

    @_host_side
    def item_weights(self, item_ids, top_k: int = 10, return_scores: bool = False):
        """The top_k largest weights of row B[i, :] for each of several items (the reference's EASE.get_similarity): an
        (n, k) int64 CPU tensor of original item ids, k = min(top_k, n_items); with return_scores also the (n, k) fp32
        weights.  Order: weight descending, ties by ascending item row; the item itself is never returned, so the
        positions beyond the n_items - 1 other items hold id -1 and weight -inf.  B[i, j] is what having item i adds to
        the score of item j.  On an itemknn model the rows are the stored neighbour lists (already in that order): k
        beyond the model's K gives id -1 / weight -inf.  An unknown id raises IndexError; another net_type ValueError."""
        if self.net_type not in ('ease', 'itemknn'):
            raise ValueError(f"item_weights needs net_type='ease' or 'itemknn', not {self.net_type!r}: call "
                             f"similar_items()")
        index = getattr(self.data_processor, "item_index", None)
        qlist = item_ids.tolist() if hasattr(item_ids, "tolist") else list(item_ids)
        k = min(int(top_k), self.n_items)
        if k <= 0 or not qlist:
            return self._empty_topk(len(qlist), k, return_scores)
        if self.net_type == 'itemknn':  # the stored lists are already in key order, without the item itself
            nbr_ids, nbr_w = self.net.neighbours()
            queries = self._dense_rows(qlist, index, self.n_items, 'item').to(nbr_ids.device)
            K = nbr_ids.shape[1]
            ids = torch.full((queries.numel(), k), -1, dtype=torch.int64)
            scores = torch.full((queries.numel(), k), float('-inf'), dtype=torch.float32)
            got = nbr_ids[queries, :min(k, K)].cpu().to(torch.int64)
            ids[:, :got.shape[1]] = got
            scores[:, :got.shape[1]] = torch.where(got >= 0, nbr_w[queries, :min(k, K)].cpu(),
                                                   torch.full((), float('-inf')))
            ids = self._original_ids(ids, index)
            return (ids, scores) if return_scores else ids
        B = self.net.weights()
        dev = B.device
        queries = self._dense_rows(qlist, index, self.n_items, 'item').to(dev)
        n = queries.numel()
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        for s in range(0, n, self.GENERIC_CHUNK):
            qs = queries[s:s + self.GENERIC_CHUNK]
            g = qs.numel()
            rows = B[qs].contiguous()
            rows[torch.arange(g, device=dev), qs] = float('-inf')
            ids[s:s + g], scores[s:s + g] = self._topk_rows(rows, rows, k, torch.full((g,), self.n_items - 1, device=dev))
        ids = self._original_ids(ids.cpu(), index)
        return (ids, scores.cpu()) if return_scores else ids

    # ------------------------------------------------------------------------------------------------ evaluate
    @_host_side
    def evaluate(self, batch_size=512, eval_metrics=['loss', 'auc']):
        """reference model.py:292-338: eval-mode scores of the test split, hinge loss and pairwise AUC per batch,
        unweighted means over batches, printed; returns None.  The printed values are kept at full precision in
        `self.eval_results` ({'loss': ..., 'auc': ...}, this rank's view of the means)."""
        self._refuse_ease("evaluate() (a pairwise loss over sampled negatives)",
                          "call evaluate_ranking() or evaluate_ranks()")
        self.net = self.net.eval()
        if self.data_processor.test_data.get('user_id', torch.empty(0)).numel() == 0:
            print("|--- No test data to evaluate.")
            return
        data = self._rank_rows(self.data_processor.test_data)
        n_test = data['user_id'].numel()
        dev = _device()
        loader = FastDataLoader(data=data, batch_size=batch_size, shuffle=False,
                                dynamic_neg_sampling=self.dynamic_neg_sampling, n_items=self.n_items,
                                item_to_metadata_map=self.data_processor.item_meta_table,
                                metadata_id_cols=self.metadata_name)
        nb = loader.num_batches
        loss_sums = torch.zeros(nb, dtype=torch.float32, device=dev)
        auc_counts = torch.zeros(nb, dtype=torch.int32, device=dev)
        if self.rng == 'reference':
            iter(loader)
            ep = self._host_epoch(data, loader)
        else:
            st = self._device_stream('test')
            sample_seed = _mix64(self.seed, 0xE7A1)
        # Linear / FM score triples independently of their batch: several batches per launch (ids, scores, per-batch
        # reductions, one id-range check per group); the MLP's activations are per batch
        # fit(loss='softmax'): every test batch is its own softmax, one batch at a time
        obj = self._objective
        softmax = obj.kind == 'softmax'
        if obj.kind == 'multineg':  # the same loss over K candidates of the evaluation sampler's rules
            self._evaluate_candidates(obj.K, st, sample_seed, nb, batch_size, n_test, lambda ids, b, err: (
                ops.score_multi_fwd_bwd(self.net.NET, self.net.tables(), ids['user'], ids['items'], ids.get('meta'),
                                        obj.loss_id, obj.temperature, loss_sums[b:b + 1], auc_counts[b:b + 1],
                                        err_flag=err, forward_only=True)))
        elif obj.kind == 'warp':
            weights = ops.warp_rank_weights(self.n_items, obj.K, obj.rank_weight, dev)
            self._evaluate_candidates(obj.K, st, sample_seed, nb, batch_size, n_test, lambda ids, b, err: (
                ops.score_warp_fwd_bwd(self.net.NET, self.net.tables(), ids['user'], ids['items'], ids.get('meta'),
                                       obj.margin, weights, loss_sums[b:b + 1], auc_counts[b:b + 1], err_flag=err,
                                       forward_only=True, want_trials=False)))
        group = 64 if hasattr(self.net, 'table_params') and not softmax else 1
        group = max(1, min(group, (1 << 22) // max(batch_size, 1)))
        if softmax:
            sm_loss = torch.zeros(nb, dtype=torch.float32, device=dev)
            sm = ops.InBatchSoftmax(min(batch_size, n_test), self.n_factors, dev)
            err = torch.zeros(1, dtype=torch.int32, device=dev)
        for b0 in (range(0, nb, group) if obj.kind in ('pair', 'softmax') else ()):
            b1 = min(b0 + group, nb)
            s, e = b0 * batch_size, min(b1 * batch_size, n_test)
            if self.rng == 'reference':
                ids = {k: v[s:e] for k, v in ep.items()}
            else:
                ids = ops.batch_prepare(st['user'], st['pos'], st['neg'], 0, s, e - s, self.n_items, sample_seed, s,
                                        st['item_meta'], sampler=self._eval_sampler())
            pos, neg = self.net.score_ids(ids)
            ops.hinge_auc_batches(pos, neg, batch_size, loss_sums[b0:b1], auc_counts[b0:b1], loss=obj.loss_id)
            if softmax:
                Bt, keep = ops.make_batch(ids['user'], ids['pos'], None, ids.get('pos_meta'), None, err)
                sm(self.net.NET, self.net.tables(), Bt, obj.temperature, obj.logq, sm_loss[b0:b0 + 1])
        if softmax:
            check_err_flag(err, "evaluate")
            loss_sums = sm_loss
        ls, ac = loss_sums.cpu().numpy(), auc_counts.cpu().numpy()
        sizes = [min((b + 1) * batch_size, n_test) - b * batch_size for b in range(nb)]
        results = {}
        if 'loss' in eval_metrics:
            results['loss'] = [float(np.float32(ls[b]) / np.float32(sizes[b])) for b in range(nb)]
        if 'auc' in eval_metrics:
            results['auc'] = [float(np.float32(ac[b]) / np.float32(sizes[b])) for b in range(nb)]
        world = tdist.world_info()[1]
        self.eval_results = {}  # the printed values at full precision (the method itself returns None, as the reference's)
        for metric in eval_metrics:
            values = results.get(metric, [])
            if world > 1:  # unweighted mean over all ranks' batches
                tot, cnt = tdist.allreduce_scalar_sum([float(sum(values)), float(len(values))], dev)
                value = tot / cnt if cnt else 0
            else:
                value = sum(values) / len(values) if values else 0
            self.eval_results[metric] = value
            print(f'|--- Testing {metric}: {value:.4f}')

    def _evaluate_candidates(self, K, st, sample_seed, nb, batch_size, n_test, score):
        """evaluate() after a fit on K candidates per row (n_negatives=K, loss='sampled_softmax', loss='warp'): one test
        batch of ops.batch_prepare_multi's blocks per forward-only launch score(ids, batch number, error flag), which
        adds the batch's loss sum and its AUC count, pairwise on (p, c_0)."""
        err = torch.zeros(1, dtype=torch.int32, device=st['user'].device)
        out = None
        for b in range(nb):
            s, e = b * batch_size, min((b + 1) * batch_size, n_test)
            ids = ops.batch_prepare_multi(st['user'], st['pos'], 0, s, e - s, self.n_items, sample_seed, s, K,
                                          st['item_meta'], out if e - s == batch_size else None,
                                          sampler=self._eval_sampler())
            if e - s == batch_size:
                out = ids
            score(ids, b, err)
        check_err_flag(err, "evaluate")

    # ------------------------------------------------------------------------------------------------ predict
    @_host_side
    def predict(self, user_id: int, top_k: int = 10, prediction_batch_size: int = 4096):
        """Top-K item ids for one user (reference model.py:341-452): score every item, sort descending, first top_k.
        Ties are ordered by ascending item id (unspecified in the reference).  Returns an int64 CPU tensor.
        `prediction_batch_size` is accepted for compatibility; the fused kernel streams the item table once and the
        result does not depend on it."""
        self.net = self.net.eval()
        scores = self.net.score_all_items(self._dense_user(user_id), self._item_meta_dev())
        k = min(int(top_k), self.n_items)
        if k <= 0:
            return torch.empty(0, dtype=torch.int64)
        return self._original_items(ops.topk(scores, k).cpu())

    def _dense_user(self, user_id):
        """Table row of a caller's user id (identity unless the ingest re-mapped ids, TensorProcessData(remap_ids=True))."""
        idx = getattr(self.data_processor, "user_index", None)
        if idx is None:
            return int(user_id)
        pos = int(torch.searchsorted(idx, torch.tensor(int(user_id), dtype=idx.dtype, device=idx.device)))
        if pos >= idx.numel() or int(idx[pos]) != int(user_id):
            raise IndexError(f"user id {user_id} does not occur in the ingested interactions")
        return pos

    def _original_items(self, rows):
        idx = getattr(self.data_processor, "item_index", None)
        return rows if idx is None else idx.cpu()[rows].to(torch.int64)


    @_host_side
    def predict_many(self, user_ids, top_k: int = 10):
        """Extension: predict() for several users — row r of the (len(user_ids), top_k) int64 CPU tensor
        equals `predict(user_ids[r], top_k)`; the per-user kernels are queued back to back and read back once."""
        self.net = self.net.eval()
        k = min(int(top_k), self.n_items)
        users = [self._dense_user(u) for u in (user_ids.tolist() if hasattr(user_ids, "tolist") else user_ids)]
        if k <= 0 or not users:
            return torch.empty((len(users), max(k, 0)), dtype=torch.int64)
        meta = self._item_meta_dev()
        out = torch.empty((len(users), k), dtype=torch.int64, device=_device())
        for r, u in enumerate(users):
            out[r] = ops.topk(self.net.score_all_items(u, meta), k)
        return self._original_items(out.cpu())

    # ------------------------------------------------------------------------------------------------ retrieval
    RECOMMEND_CHUNK = 65_536  # query users per fused call: bounds the workspace ((512 + n/32) * 32 * k * 8 bytes)
    GENERIC_CHUNK = 16        # score rows per pass of the generic path (MLP, k > KMAX)

    def _dense_users(self, user_ids):
        """Table rows of a list of caller user ids (vectorised _dense_user); IndexError on an unknown id."""
        ids = torch.as_tensor(user_ids.tolist() if hasattr(user_ids, "tolist") else list(user_ids), dtype=torch.int64)
        ids = ids.reshape(-1)
        idx = getattr(self.data_processor, "user_index", None)
        if idx is None:
            bad = (ids < 0) | (ids >= self.n_users)
            if bool(bad.any()):
                raise IndexError(f"user id {int(ids[bad][0])} outside [0, {self.n_users})")
            return ids
        idx = idx.cpu().to(torch.int64)
        pos = torch.searchsorted(idx, ids)
        ok = pos < idx.numel()
        ok[ok.clone()] = idx[pos[ok]] == ids[ok]
        if not bool(ok.all()):
            raise IndexError(f"user id {int(ids[~ok][0])} does not occur in the ingested interactions")
        return pos

    def _fused_retrieval(self, k):
        return hasattr(self.net, 'table_params') and k <= ops._lib.RETRIEVE_KMAX and \
            self.n_factors <= ops._lib.RETRIEVE_DMAX

    @staticmethod
    def _empty_topk(n, k, return_scores):
        """What recommend() and its kin return when there is no query or k <= 0: (n, max(k, 0)) ids (and scores)."""
        e = torch.empty((n, max(k, 0)), dtype=torch.int64)
        return (e, torch.empty(e.shape, dtype=torch.float32)) if return_scores else e

    def _chunked(self, call, queries):
        """call(chunk) -> tuple of tensors (or None) per RECOMMEND_CHUNK of `queries`: the tuple of concatenations.
        `queries` is not empty (the callers return _empty_topk first)."""
        assert queries.numel() > 0
        outs = [call(queries[s:s + self.RECOMMEND_CHUNK]) for s in range(0, queries.numel(), self.RECOMMEND_CHUNK)]
        return tuple(None if o[0] is None else torch.cat(o) for o in zip(*outs))

    @staticmethod
    def _original_ids(ids, index):
        """Dense ids (CPU tensor, changed in place) -> the caller's ids through `index` (None: the same); -1 stays."""
        if index is not None:
            keep = ids >= 0
            ids[keep] = index.cpu().to(torch.int64)[ids[keep]]
        return ids

    @staticmethod
    def _topk_rows(rows, out_rows, k, n_valid):
        """Tail of the generic paths: ops.topk of each score row, out_rows' values there, and id -1 / score -inf from
        position n_valid[r] on.  (ids (g, k) int64, scores (g, k) fp32)."""
        top = torch.stack([ops.topk(rows[r], k) for r in range(rows.shape[0])])
        sc = torch.gather(out_rows, 1, top)
        pad = torch.arange(k, device=rows.device)[None, :] >= n_valid[:, None]
        return torch.where(pad, torch.full_like(top, -1), top), torch.where(pad, torch.full_like(sc, float('-inf')), sc)

    def _generic_form(self, dev, meta):
        """What the generic path's score rows rank by: (S, c, table parameters) of the folded form for Linear / FM up to
        TRS_RETRIEVE_DMAX factors; None (the scorer's own score_all_items rows) for the MLP and wider tables."""
        if not hasattr(self.net, 'table_params'):
            return None
        fold = ops.item_fold(self.net.NET, self.net.tables(), self.n_items, self.n_factors, dev, meta)
        if fold is None:
            return None
        S, c = ops.fold_views(fold, self.n_items, self.n_factors)
        return S, c, self.net.table_params()

    def _generic_rows(self, us, meta, form):
        """Score rows of the dense users `us` (a GENERIC_CHUNK of them): (rows ranked by, rows in output units)."""
        dev = us.device
        if hasattr(self.net, 'score_rows'):  # EASE: the chunk's rows in one launch
            rows = self.net.score_rows(us)
            return rows, rows
        if form is None:
            rows = torch.stack([self.net.score_all_items(int(u), meta) for u in us.tolist()])
            return rows, rows
        S, c, tp = form
        Ut = torch.zeros((us.numel(), S.shape[1]), dtype=torch.float32, device=dev)
        Ut[:, :self.n_factors] = tp[0].data[us]
        Tz, keep = ops.make_tables(Ut, S, tp[2].data[us].contiguous(), c.view(-1, 1))
        rows = torch.stack([ops.score_all_items("linear", Tz, r, self.n_items, dev) for r in range(us.numel())])
        out_rows = rows if self.net.NET == "linear" else \
            torch.stack([self.net.score_all_items(int(u), meta) for u in us.tolist()])
        return rows, out_rows

    def _rank_dense(self, users, k, exclude_seen, rel=None, fold=None):
        """Top-k of dense users (int64 GPU tensor): (ids (n,k) dense int64 with -1 padding, scores (n,k) fp32, metrics
        (n,4) float64 or None).  Linear / FM with k <= KMAX: the fused kernel; otherwise score rows + mask + top-k.
        fold: the item fold of the current tables when the caller has built it already (fused path only)."""
        dev = users.device
        seen = self._seen_csr() if exclude_seen else None
        meta = self._item_meta_dev()
        n = users.numel()
        if self._fused_retrieval(k):
            T = self.net.tables()
            if fold is None:
                fold = ops.item_fold(self.net.NET, T, self.n_items, self.n_factors, dev, meta)
            return self._chunked(lambda us: ops.retrieve_topk(self.net.NET, T, fold, us, k, seen, rel), users)
        # generic path: existing score rows, seen entries -> -inf, trs_topk, -1 beyond the user's unseen items.
        # Linear / FM rank the rows of the folded form (Linear scores, FM logits z: score_all_items of a Linear scorer
        # over S / c with the users' rows padded to Dp); FM's returned scores are its own sigmoid rows.
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        form = self._generic_form(dev, meta)
        for s in range(0, n, self.GENERIC_CHUNK):
            us = users[s:s + self.GENERIC_CHUNK]
            rows, out_rows = self._generic_rows(us, meta, form)
            if seen is not None:
                ops.mask_seen(rows, us, seen)
                n_seen = (seen[0][us + 1] - seen[0][us])
            else:
                n_seen = torch.zeros_like(us)
            ids[s:s + us.numel()], scores[s:s + us.numel()] = self._topk_rows(rows, out_rows, k, self.n_items - n_seen)
        met = ops.rank_metrics(ids, users, rel) if rel is not None and n else None
        return ids, scores, met

    @_host_side
    def recommend(self, user_ids, top_k: int = 10, exclude_seen: bool = True, return_scores: bool = False):
        """Top-k item ids of several users at once: an (n, k) int64 CPU tensor of original item ids, k = min(top_k,
        n_items); with return_scores also the (n, k) fp32 scores in the scorer's output units.  exclude_seen drops the
        items each user has in the train split; a user with fewer than k other items gets id -1 / score -inf in the
        remaining positions.  Ties are ordered by ascending item id as in predict().
        Linear and FM (k <= TRS_RETRIEVE_KMAX, D <= TRS_RETRIEVE_DMAX) run one fused fp32 matrix-core kernel over user
        tiles x item tiles with the top-k selection in its epilogue; the MLP and larger k score rows one user at a time.
        FM ranks by the logit z before its sigmoid: this is the one place where the order can differ from predict(),
        which sorts the fp32 sigmoid values (equal where the sigmoid saturates; recommend keeps z's order there).
        Scores may differ from predict()'s in the last bits (another summation order over the factors)."""
        self.net = self.net.eval()
        ulist = user_ids.tolist() if hasattr(user_ids, "tolist") else list(user_ids)
        k = min(int(top_k), self.n_items)
        if k <= 0 or not ulist:
            return self._empty_topk(len(ulist), k, return_scores)
        users = self._dense_users(ulist).to(_device())
        ids, scores, _ = self._rank_dense(users, k, exclude_seen)
        ids = self._original_ids(ids.cpu(), getattr(self.data_processor, "item_index", None))
        return (ids, scores.cpu()) if return_scores else ids

    # ------------------------------------------------------------------------------------------------ exact ranks
    RANK_TARGET_BLOCK = 1024  # targets per compare block of the generic path: (block, n_items) booleans

    @staticmethod
    def _group_pairs(du, di, n_items):
        """Distinct (dense user, dense item) pairs sorted by (user, item), as a query list with a query-indexed CSR:
        (query users (n_q,), offsets (n_q + 1,), items (n_t,), inverse (n,)), all int64 — input pair j is CSR entry
        inverse[j], so duplicate pairs share one entry."""
        uniq, inv = torch.unique(du * int(n_items) + di, return_inverse=True)
        pu = torch.div(uniq, int(n_items), rounding_mode="floor")
        qusers, counts = torch.unique_consecutive(pu, return_counts=True)
        off = torch.zeros(qusers.numel() + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(counts, 0)
        return qusers, off, uniq - pu * int(n_items), inv

    def _ranks_dense(self, qusers, off, items, exclude_seen, want_values=False):
        """Exact ranks of a query-indexed CSR of dense targets (int64 tensors: query users (n_q,), offsets (n_q + 1,),
        sorted distinct items per row): (ranks (n_t,) int64 CPU, values (n_t,) fp32 CPU in output units or None).
        Linear / FM up to TRS_RETRIEVE_DMAX factors: trs_item_ranks per RECOMMEND_CHUNK of queries; otherwise the
        generic path's score rows, the targets' values read before the seen entries become -inf, and a count of
        (row > v_t) | ((row == v_t) & (id < t)) per target."""
        dev = _device()
        seen = self._seen_csr() if exclude_seen else None
        meta = self._item_meta_dev()
        off = off.cpu()
        nq = qusers.numel()
        ranks = torch.empty(items.numel(), dtype=torch.int64, device=dev)
        values = torch.empty(items.numel(), dtype=torch.float32, device=dev) if want_values else None
        qusers, items = qusers.to(dev), items.to(dev)
        if hasattr(self.net, 'table_params') and self.n_factors <= ops._lib.RETRIEVE_DMAX:
            T = self.net.tables()
            fold = ops.item_fold(self.net.NET, T, self.n_items, self.n_factors, dev, meta)
            for s in range(0, nq, self.RECOMMEND_CHUNK):
                e = min(s + self.RECOMMEND_CHUNK, nq)
                lo, hi = int(off[s]), int(off[e])
                r, v = ops.item_ranks(self.net.NET, T, fold, qusers[s:e].contiguous(),
                                      ((off[s:e + 1] - lo).to(dev), items[lo:hi].to(torch.int32).contiguous()), seen,
                                      want_values)
                ranks[lo:hi] = r
                if want_values:
                    values[lo:hi] = v
            return ranks.cpu(), values.cpu() if want_values else None
        form = self._generic_form(dev, meta)
        ar = torch.arange(self.n_items, device=dev)
        for s in range(0, nq, self.GENERIC_CHUNK):
            us = qusers[s:s + self.GENERIC_CHUNK]
            rows, out_rows = self._generic_rows(us, meta, form)
            segs = [(int(off[s + r]), int(off[s + r + 1])) for r in range(us.numel())]
            vts = [rows[r, items[lo:hi]] for r, (lo, hi) in enumerate(segs)]  # before masking: a target may be seen
            if want_values:
                for r, (lo, hi) in enumerate(segs):
                    values[lo:hi] = out_rows[r, items[lo:hi]]
            if seen is not None:
                ops.mask_seen(rows, us, seen)
            for r, (lo, hi) in enumerate(segs):
                for b in range(lo, hi, self.RANK_TARGET_BLOCK):
                    t = items[b:min(b + self.RANK_TARGET_BLOCK, hi)]
                    vt = vts[r][b - lo:b - lo + t.numel()][:, None]
                    row = rows[r][None, :]
                    ranks[b:b + t.numel()] = ((row > vt) | ((row == vt) & (ar[None, :] < t[:, None]))).sum(1)
        return ranks.cpu(), values.cpu() if want_values else None

    @_host_side
    def rank_items(self, user_ids, item_ids, exclude_seen: bool = True, return_scores: bool = False):
        """Where item_ids[j] lands in the full ranking of user_ids[j]: an (n,) int64 CPU tensor of 0-based ranks in
        input order; with return_scores also the (n,) fp32 values in the scorer's output units (as recommend()).
        rank = the number of candidate items other than the target that recommend() orders before it: value descending
        (Linear score, FM logit z), ties by ascending item id.  Candidates are all items, with exclude_seen without the
        user's train items; a target that is itself a train item is ranked as if it were a candidate, and the user's
        other targets compete like any other item.  For a candidate target and top_k <= TRS_RETRIEVE_KMAX,
        recommend(u, top_k, exclude_seen)[r] == t exactly when rank_items([u], [t], exclude_seen) == r: the kernel computes
        the target's value with the instruction sequence recommend()'s tile loop uses.
        Unequal lengths raise ValueError, an unknown user or item IndexError; duplicate pairs get the same answer.
        Linear and FM up to TRS_RETRIEVE_DMAX factors run one more pass of recommend()'s matrix-core tile loop whose
        epilogue counts the items above each target; the MLP and wider tables count over score rows one user at a time."""
        self.net = self.net.eval()
        ulist = user_ids.tolist() if hasattr(user_ids, "tolist") else list(user_ids)
        ilist = item_ids.tolist() if hasattr(item_ids, "tolist") else list(item_ids)
        if len(ulist) != len(ilist):
            raise ValueError(f"rank_items takes as many item ids as user ids, got {len(ulist)} and {len(ilist)}")
        if not ulist:
            e = torch.empty(0, dtype=torch.int64)
            return (e, torch.empty(0, dtype=torch.float32)) if return_scores else e
        du = self._dense_users(ulist)
        di = self._dense_rows(ilist, getattr(self.data_processor, "item_index", None), self.n_items, 'item')
        qusers, off, items, inv = self._group_pairs(du, di, self.n_items)
        ranks, values = self._ranks_dense(qusers, off, items, exclude_seen, return_scores)
        return (ranks[inv], values[inv]) if return_scores else ranks[inv]

    @_host_side
    def evaluate_ranks(self, k=(1, 10, 100), metrics=('auc', 'mrr', 'precision', 'recall', 'ndcg', 'map'),
                       exclude_seen: bool = True, users=None):
        """Rank-aware metrics over the full catalogue against the test split, from the exact rank of every (user,
        held-out item) pair (rank_items); returns {'auc': .., 'mrr': .., 'precision@10': .., .., 'n_users': int} and
        prints the entries as evaluate_ranking() does.
        Users, T_u (the user's distinct test items, without its train items when exclude_seen) and the candidates C_u are
        those of evaluate_ranking(); users with an empty T_u, or whose candidates are all relevant, are skipped.
        metrics: 'auc', 'mrr', 'mean_rank' and, for every k (an int or a sequence of ints >= 1, no upper limit; k >
        n_items behaves as n_items), 'hit_rate', 'precision', 'recall', 'ndcg', 'map' — the formulas are in
        evaluate/ranks.py.  Per-user values in float64, averaged over the evaluated users in ascending user order.
        Data parallel: as evaluate_ranking() (users with user_id % world == rank, sums all-reduced)."""
        ks = [int(k)] if isinstance(k, (int, np.integer)) else [int(x) for x in k]
        metrics = [metrics] if isinstance(metrics, str) else list(metrics)
        rank_eval.check(metrics, ks)
        rank, world = tdist.world_info()
        if world > 1 and (getattr(self, 'pre_sharded', False) or self.dp_partition != 'user'):
            raise ValueError("evaluate_ranks under data parallelism needs dp_partition='user' without pre_sharded: "
                             "a rank must hold every train and test row of the users it evaluates")
        self.net = self.net.eval()
        dev = _device()
        roff, ritems = self._relevance_csr(exclude_seen)
        if users is None:
            dense = torch.unique(self.data_processor.test_data['user_id'].to(torch.int64))
        else:
            dense = torch.unique(self._dense_users(users))
        if world > 1:
            dense = dense[dense % world == rank]
        dense = dense.to(dev)
        cnt = roff[dense + 1] - roff[dense]
        dense, cnt = dense[cnt > 0], cnt[cnt > 0]
        names = rank_eval.entries(metrics, ks)
        sums = np.zeros(len(names) + 1)
        if dense.numel():
            n_c = torch.full_like(cnt, self.n_items)
            if exclude_seen:
                soff = self._seen_csr()[0]
                n_c -= soff[dense + 1] - soff[dense]
            off = torch.zeros(dense.numel() + 1, dtype=torch.int64, device=dev)
            off[1:] = torch.cumsum(cnt, 0)
            within = torch.arange(int(off[-1]), device=dev) - torch.repeat_interleave(off[:-1], cnt)
            items = ritems[torch.repeat_interleave(roff[dense], cnt) + within].to(torch.int64)
            ranks, _ = self._ranks_dense(dense, off, items, exclude_seen)
            keep, per = rank_eval.per_user(ranks.numpy(), off.cpu().numpy(), n_c.cpu().numpy(), ks, metrics,
                                           self.n_items)
            sums = np.array([float(np.sum(per[name])) for name in names] + [float(keep.sum())])
        if world > 1:
            sums = np.array(tdist.allreduce_scalar_sum(sums.tolist(), dev))
        n = int(sums[-1])
        results = {}
        for j, name in enumerate(names):
            value = float(sums[j] / n) if n else 0.0
            results[name] = value
            print(f'|--- Testing {name}: {value:.4f}')
        results['n_users'] = n
        return results

    # ------------------------------------------------------------------------------------------------ fold-in
    def _check_fold_in(self, what, epochs, lr, loss, l2, seed, max_tries, reject_seen):
        """Argument checks of fold_in_users / recommend_for_histories (before any device work)."""
        self._refuse_ease(f"{what}()", "call recommend_for_histories(), which needs no fitting with EASE", ValueError)
        if self.net_type not in ('linear', 'fm'):
            raise ValueError(f"{what} needs net_type 'linear' or 'fm': with net_type={self.net_type!r} (mlp) a user is "
                             "not an inner-product row against a folded item matrix")
        if self.n_factors > ops._lib.RETRIEVE_DMAX:
            raise ValueError(f"{what} takes n_factors <= {ops._lib.RETRIEVE_DMAX} (TRS_RETRIEVE_DMAX), got "
                             f"{self.n_factors}")

        def integer(v, name, lo, hi):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} must be an integer in {lo}..{hi}, got {v!r}")

        def number(v, name, positive):
            ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(v)
            if not ok or (v <= 0 if positive else v < 0):
                raise ValueError(f"{name} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
        integer(epochs, "epochs", 1, 1024)
        number(lr, "lr", True)
        number(l2, "l2", False)
        if loss not in ('hinge', 'bpr'):
            raise ValueError(f"loss must be 'hinge' or 'bpr', got {loss!r}")
        integer(seed, "seed", -(1 << 63), (1 << 64) - 1)
        integer(max_tries, "max_tries", 0, 64)
        if reject_seen and int(max_tries) < 1:
            raise ValueError("reject_seen needs max_tries >= 1")

    def _history_csr(self, histories, side='item'):
        """Host side of fold-in: original item ids -> dense rows (IndexError on an unknown id), every history sorted and
        de-duplicated, the users ordered by history length, longest first (the lane groups of a wave then have similar
        trip counts and the long tails start first).  Returns (offsets int64 (n+1,), items int32, rank) as numpy arrays:
        row rank[r] of the CSR is the caller's history r.  side='user' (fold_in_items): the histories hold user ids."""
        hs = [np.asarray(h.tolist() if hasattr(h, "tolist") else list(h), dtype=np.int64).reshape(-1) for h in histories]
        n = len(hs)
        lens = np.array([h.size for h in hs], dtype=np.int64)
        flat = np.concatenate(hs) if n and lens.sum() else np.zeros(0, dtype=np.int64)
        n_side = int(self.n_items if side == 'item' else self.n_users)
        dense = self._dense_rows(flat, getattr(self.data_processor, side + "_index", None), n_side, side).numpy()
        key = np.unique(np.repeat(np.arange(n, dtype=np.int64), lens) * n_side + dense)
        rows, items = key // n_side, key % n_side
        counts = np.bincount(rows, minlength=n).astype(np.int64)
        order = np.argsort(-counts, kind='stable')
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.arange(n, dtype=np.int64)
        off_orig = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        off = np.concatenate([[0], np.cumsum(counts[order])]).astype(np.int64)
        out = np.empty(items.size, dtype=np.int32)
        out[off[rank[rows]] + (np.arange(items.size, dtype=np.int64) - off_orig[rows])] = items
        return off, out, rank

    def _fold_in_dense(self, off, items, opts, want_loss):
        """Fold-in of a dense history CSR (numpy) on the device: (fold, (off, items) on the GPU, U, b, loss | None)."""
        dev = _device()
        self.net = self.net.eval()
        fold = ops.item_fold(self.net.NET, self.net.tables(), self.n_items, self.n_factors, dev, self._item_meta_dev())
        hist = (torch.from_numpy(off).to(dev), torch.from_numpy(items).to(dev))
        U, b, ls = ops.fold_in_users(self.net.NET, fold, self.n_items, self.n_factors, hist, opts['loss'],
                                     opts['epochs'], opts['lr'], opts['l2'], opts['seed'], opts['shuffle'],
                                     opts['reject_seen'], opts['max_tries'], want_loss=want_loss)
        return fold, hist, U, b, ls

    @_host_side
    def fold_in_users(self, histories, epochs: int = 8, lr: float = 0.05, loss: str = 'hinge', l2: float = 0.0,
                      seed: int = 0, shuffle: bool = True, reject_seen: bool = True, max_tries: int = 8,
                      return_loss: bool = False):
        """Rows for users the model has never seen, fitted to their item histories with the item side frozen: CPU
        tensors U (n, n_factors) fp32 and b (n,) fp32 — what the user table and user_bias / linear_user would hold —
        and with return_loss the (epochs, n) fp32 mean pair loss of every epoch.
        histories: a sequence of sequences / 1-D arrays of original item ids (an unknown id raises IndexError); each is
        sorted and de-duplicated first.  Per user, `epochs` passes of per-visit SGD over the history (shuffled per epoch
        when `shuffle`), one sampled negative per visit (one the history holds is redrawn, at most max_tries candidates,
        when reject_seen), loss 'hinge' or 'bpr' on the scorer's outputs, step lr, L2 coefficient l2 on u and b; the
        exact rule is in include/trs.h ("fold-in").  The result for a history does not depend on the other histories of
        the call.  An empty history gives u = 0, b = 0.  One kernel launch for all users.
        Linear and FM only (ValueError for the MLP and for n_factors > TRS_RETRIEVE_DMAX).  The model's parameters are
        never written.  Under torch.distributed every rank answers from its own replica."""
        self._check_fold_in("fold_in_users", epochs, lr, loss, l2, seed, max_tries, reject_seen)
        opts = dict(epochs=int(epochs), lr=float(lr), loss=loss, l2=float(l2), seed=int(seed), shuffle=bool(shuffle),
                    reject_seen=bool(reject_seen), max_tries=int(max_tries))
        off, items, rank = self._history_csr(histories)
        n = rank.size
        if n == 0:
            U, b = torch.empty((0, self.n_factors), dtype=torch.float32), torch.empty((0,), dtype=torch.float32)
            return (U, b, torch.empty((opts['epochs'], 0), dtype=torch.float32)) if return_loss else (U, b)
        _, _, U, b, ls = self._fold_in_dense(off, items, opts, return_loss)
        r = torch.from_numpy(rank)
        U, b = U.cpu()[r], b.cpu()[r]
        return (U, b, ls.cpu()[:, r]) if return_loss else (U, b)

    @_host_side
    def recommend_for_histories(self, histories, top_k: int = 10, exclude_seen: bool = True,
                                return_scores: bool = False, **fold_in_options):
        """recommend() for users the model has never seen: fold_in_users(histories, **fold_in_options), then the fused
        top-k of recommend() over the model's folded items with the folded-in rows as the user side.  Output as
        recommend(): an (n, k) int64 CPU tensor of original item ids, k = min(top_k, n_items), with return_scores also
        the (n, k) fp32 scores (FM: sigmoid(z), ranked by z); exclude_seen drops each history's own items; positions
        beyond the candidates hold id -1 / score -inf; ties by ascending item row.
        Only the fused kernel is offered: top_k > TRS_RETRIEVE_KMAX raises ValueError (the generic path of recommend()
        for larger k is out of scope here), as do the MLP and n_factors > TRS_RETRIEVE_DMAX."""
        if self.net_type == 'ease':
            if fold_in_options:
                raise ValueError(f"recommend_for_histories with net_type='ease' takes no fold-in options (nothing is "
                                 f"fitted: a history's scores are the sum of its items' rows of B), got "
                                 f"{sorted(fold_in_options)}")
            return self._item_item_recommend_for_histories(
                lambda hist, us: ops.ease_scores(self.net.weights(), hist, us), lambda: self.net.weights().device,
                histories, top_k, exclude_seen, return_scores)
        if self.net_type == 'itemknn':
            if fold_in_options:
                raise ValueError(f"recommend_for_histories with net_type='itemknn' takes no fold-in options (nothing is "
                                 f"fitted: a history's scores are the sums over its items' neighbour lists), got "
                                 f"{sorted(fold_in_options)}")
            return self._item_item_recommend_for_histories(
                self.net.score_csr_rows, lambda: self.net.neighbours()[0].device, histories, top_k, exclude_seen,
                return_scores)
        unknown = set(fold_in_options) - {'epochs', 'lr', 'loss', 'l2', 'seed', 'shuffle', 'reject_seen', 'max_tries'}
        if unknown:
            raise ValueError(f"unknown fold-in options {sorted(unknown)}")
        opts = dict(epochs=8, lr=0.05, loss='hinge', l2=0.0, seed=0, shuffle=True, reject_seen=True, max_tries=8)
        opts.update(fold_in_options)
        self._check_fold_in("recommend_for_histories", opts['epochs'], opts['lr'], opts['loss'], opts['l2'],
                            opts['seed'], opts['max_tries'], opts['reject_seen'])
        if int(top_k) > ops._lib.RETRIEVE_KMAX:
            raise ValueError(f"recommend_for_histories takes top_k <= {ops._lib.RETRIEVE_KMAX} (TRS_RETRIEVE_KMAX), got "
                             f"{top_k}")
        opts = dict(epochs=int(opts['epochs']), lr=float(opts['lr']), loss=opts['loss'], l2=float(opts['l2']),
                    seed=int(opts['seed']), shuffle=bool(opts['shuffle']), reject_seen=bool(opts['reject_seen']),
                    max_tries=int(opts['max_tries']))
        off, items, rank = self._history_csr(histories)
        n = rank.size
        k = min(int(top_k), self.n_items)
        if k <= 0 or n == 0:
            return self._empty_topk(n, k, return_scores)
        fold, hist, U, b, _ = self._fold_in_dense(off, items, opts, False)
        # a temporary table set whose user side is the folded-in rows: the fused kernel reads nothing else of it
        T, keep = ops.make_tables(U, self.net.item.weight.data, b.view(-1, 1), self.net.table_params()[3].data)
        users = torch.arange(n, dtype=torch.int64, device=U.device)
        seen = hist if exclude_seen and hist[1].numel() else None  # every history empty: nothing to exclude
        ids, scores, _ = self._chunked(lambda us: ops.retrieve_topk(self.net.NET, T, fold, us, k, seen), users)
        r = torch.from_numpy(rank)
        ids = self._original_ids(ids.cpu()[r], getattr(self.data_processor, "item_index", None))
        return (ids, scores.cpu()[r]) if return_scores else ids

    # ------------------------------------------------------------------------------------------------ sequence model
    _SEQ_UNFITTED = "call fit_sequence() first"

    def _check_sequence_model(self, what):
        """What every sequence call needs of the model (before any device work): a Linear net without metadata, one
        process, a row width the staging kernels take."""
        if self.net_type != 'linear' or self.use_metadata:
            kind = f"net_type={self.net_type!r}" + (" with metadata columns" if self.use_metadata else "")
            raise ValueError(f"{what} needs net_type='linear' without metadata columns, not {kind}: the sequence model "
                             "adds a context table to the Linear scorer's rows ('fm', 'mlp', 'ease' and metadata are "
                             "out of scope)")
        if tdist.world_info()[1] > 1:
            raise NotImplementedError(f"{what} runs in a single process: under torch.distributed (world > 1) a rank "
                                      "holds a shard of the interactions, not whole user sequences")
        D = int(self.n_factors)
        if D < 1 or D > 1024 or (D % 4 != 0 and D > 256):
            raise ValueError(f"{what}: n_factors={D} is not a row width the kernels take (1..1024; not a multiple of 4 "
                             "only up to 256)")

    def _sequence_buffers(self, what):
        C, w = getattr(self.net, "seq_context", None), getattr(self.net, "seq_weights", None)
        if C is None or w is None:
            raise RuntimeError(f"{what}: {self._SEQ_UNFITTED}")
        return C, w

    def _check_sequence_topk(self, what, top_k):
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)):
            raise ValueError(f"{what}: top_k must be an integer, got {top_k!r}")
        if int(top_k) > ops._lib.RETRIEVE_KMAX:
            raise ValueError(f"{what} takes top_k <= {ops._lib.RETRIEVE_KMAX} (TRS_RETRIEVE_KMAX), got {top_k}")
        if self.n_factors > ops._lib.RETRIEVE_DMAX:
            raise ValueError(f"{what} takes n_factors <= {ops._lib.RETRIEVE_DMAX} (TRS_RETRIEVE_DMAX), got "
                             f"{self.n_factors}")

    def _check_timestamps(self, what, timestamps):
        """timestamps as a 1-D CPU tensor with one finite number per INPUT row (None stays None); ValueError otherwise."""
        if timestamps is None:
            return None
        timestamps = torch.as_tensor(np.asarray(timestamps.cpu() if hasattr(timestamps, "cpu") else timestamps))
        n_in = self.data_processor.n_input_rows
        if timestamps.dim() != 1 or timestamps.numel() != n_in or timestamps.dtype == torch.bool:
            raise ValueError(f"{what}: timestamps must hold one number per input row ({n_in}), got shape "
                             f"{tuple(timestamps.shape)}")
        if timestamps.is_floating_point() and not bool(torch.isfinite(timestamps).all()):
            raise ValueError(f"{what}: timestamps must be finite")
        return timestamps

    def _sequences(self, timestamps=None):
        """The ordered per-user CSR of the train split on the device.  Built on first use, by input position or by the
        timestamps given then; built again whenever timestamps are given.  The order is the MODEL OBJECT's, not the
        tables': it is not part of state_dict() (set_sequence_order())."""
        if 'sequences' not in self._dev_cache or timestamps is not None:
            st = self._device_stream('train')
            dev = st['user'].device
            rows = self.data_processor.train_rows().to(dev)
            ts = None if timestamps is None else timestamps.to(dev)
            self._dev_cache['sequences'] = ordered_sequences(st['user'], st['pos'], rows, self.n_users, ts)
        return self._dev_cache['sequences']

    @_host_side
    def set_sequence_order(self, timestamps=None):
        """Fixes the order of every user's train sequence for the sequence calls: by `timestamps` (one number per INPUT
        row, ties by input position), or with None by input position.  fit_sequence(timestamps=...) does the same.  The
        order stays with this model object until it is set again: a later fit_sequence() without timestamps keeps
        training on it, and recommend_next() / evaluate_next() read each user's last items from it.  It is NOT part of
        state_dict(): a model restored from one orders by input position until this is called with the timestamps the
        context table was fitted on.  A held-out set of an earlier fit_sequence(holdout_last=True) is dropped (its
        positions belong to the old order)."""
        what = "set_sequence_order"
        self._check_sequence_model(what)
        timestamps = self._check_timestamps(what, timestamps)
        _device()
        self._dev_cache.pop('sequences', None)
        self._seq_holdout = None
        self._sequences(timestamps)

    @_host_side
    def fit_sequence(self, epochs: int = 10, lr: float = 0.05, batch_size: int = 4096, context: int = 4,
                     decay: float = 0.7, loss: str = 'bpr', seed: int = 0, timestamps=None, holdout_last: bool = False,
                     return_loss: bool = False):
        """Next-item training over each user's ORDERED train sequence: a factorised Markov model over the last `context`
        items (FPMC for context = 1, the Fossil family beyond) on the Linear scorer's tables U, V, b plus one context
        table C (n_items, n_factors).  For position k of user u's sequence s_u,
            q = U[u] + sum_{l < min(context, k)} w_l C[s_u[k-1-l]],    z(i) = <q, V[i]> + b[i],
        w_l = decay^l / sum_{j < context} decay^j (l = 0 the most recent item), and the row loss is 'bpr' or 'hinge' on
        (z(s_u[k]), z(a sampled negative)); the exact rule is in include/trs.h "sequence model".  C starts as zeros: a
        fresh model is exactly the Linear model it was.
        Order: the input row position, ascending; `timestamps` (one number per INPUT row, train and test rows alike, of
        either front door) overrides it, ties broken by row position.  Repeated items stay in the sequences.  The order
        stays with the model object: a later call WITHOUT timestamps keeps the order of the last call that gave some,
        and it is not part of state_dict() (set_sequence_order() sets it on a restored model, or resets it).
        holdout_last keeps every user's last train interaction out of training and remembers it for evaluate_next();
        users with fewer than two interactions hold out nothing.
        Every epoch visits every remaining position once, in a permutation seeded by (seed, epoch); one step = a
        negative per row (uniform, never the row's positive), one staging launch (trs_seq_fwd_bwd) and plain SGD at
        `lr` on the rows it references.  No optimiser object, no host sync inside an epoch.
        C and the weights become buffers of the net (state_dict() carries them).  A second call continues from the
        current tables; another `context` or `decay` then raises.  U, V, b are written in place: recommend(),
        similar_items(), evaluate() and the rest keep answering from the context-free Linear model those tables are.
        Returns None, or with return_loss the (epochs,) float64 mean row loss of every epoch.
        Before any device work: ValueError for another net_type, metadata, or a bad argument; NotImplementedError under
        torch.distributed with more than one rank."""
        what = "fit_sequence"
        self._check_sequence_model(what)

        def integer(v, name, lo, hi=None):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
                raise ValueError(f"{what}: {name} must be an integer in {lo}..{'' if hi is None else hi}, got {v!r}")
            return int(v)

        def positive(v, name):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                    not (math.isfinite(v) and v > 0):
                raise ValueError(f"{what}: {name} must be a finite number > 0, got {v!r}")
            return float(v)

        epochs, batch_size = integer(epochs, "epochs", 1), integer(batch_size, "batch_size", 1)
        L = integer(context, "context", 0, ops._lib.SEQ_LMAX)
        seed = integer(seed, "seed", 0)
        lr, decay = positive(lr, "lr"), positive(decay, "decay")
        if loss not in ('bpr', 'hinge'):
            raise ValueError(f"{what}: loss must be 'bpr' or 'hinge', got {loss!r}")
        if self.n_items < 2:
            raise ValueError(f"{what}: sampling a negative needs n_items >= 2")
        timestamps = self._check_timestamps(what, timestamps)
        weights = ops.seq_weights(L, decay)
        C, w = getattr(self.net, "seq_context", None), getattr(self.net, "seq_weights", None)
        if C is not None and w is not None and not (w.numel() == L and torch.equal(w.cpu(), weights)):
            raise ValueError(f"{what}: the model already has a context table fitted with other slot weights "
                             f"({w.cpu().tolist()}); context={L}, decay={decay} would give {weights.tolist()}")
        dev = _device()
        self.net = self.net.train()
        off, ids = self._sequences(timestamps)
        if C is None or w is None:
            self.net.seq_context = torch.zeros((self.n_items, self.n_factors), dtype=torch.float32, device=dev)
            self.net.seq_weights = weights.to(dev)
        C, w = self.net.seq_context, self.net.seq_weights
        entries, held_users, held_pos = sequence_entries(off, holdout_last)
        self._seq_holdout = (held_users, held_pos) if holdout_last else None
        n = int(entries.numel())
        loss_sums = torch.zeros(epochs, dtype=torch.float32, device=dev)
        if n:
            from .engine import SequenceTrainer
            B = min(batch_size, n)
            trainer = SequenceTrainer(self.net, C, w, (off, ids), B, lr, ops._lib.LOSS_ID[loss])
            user_of = torch.repeat_interleave(torch.arange(self.n_users, dtype=torch.int32, device=dev),
                                              off[1:] - off[:-1])
            done = getattr(self, "_seq_epochs_done", 0)
            with torch.no_grad():
                for ep in range(epochs):
                    g = torch.Generator(device=dev)
                    g.manual_seed(_mix64(seed, done + ep) & (2 ** 63 - 1))
                    ent = entries[torch.randperm(n, device=dev, generator=g)]
                    usr = user_of[ent]
                    sample_seed = _mix64(seed ^ 0x5EC0DE, done + ep)
                    for s in range(0, n, B):
                        trainer.seq_step(usr[s:s + B], ent[s:s + B], loss_sums[ep:ep + 1], sample_seed, s)
                    avg = float(loss_sums[ep].item()) / n  # the epoch's one read
                    print(f'|--- Epoch {ep+1}/{epochs} --- Training Loss: {avg:.4f}')
            self._seq_epochs_done = done + epochs
            trainer.check_errors()
        return (loss_sums.cpu().to(torch.float64) / max(n, 1)) if return_loss else None

    @staticmethod
    def _gather_csr(off, items, rows, drop_last=0):
        """Rows `rows` (int64, same device) of a CSR as a CSR of their own, each without its last drop_last entries."""
        cnt = (off[rows + 1] - off[rows] - int(drop_last)).clamp_(min=0)
        noff = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=off.device)
        noff[1:] = torch.cumsum(cnt, 0)
        within = torch.arange(int(noff[-1]), device=off.device) - torch.repeat_interleave(noff[:-1], cnt)
        return noff, items[torch.repeat_interleave(off[rows], cnt) + within].contiguous()

    @staticmethod
    def _distinct_csr(off, items, n_items):
        """The sorted, distinct items of every row of a CSR (what the retrieval kernels take as a seen list)."""
        n = off.numel() - 1
        row = torch.repeat_interleave(torch.arange(n, device=off.device), off[1:] - off[:-1])
        key = torch.unique(row * int(n_items) + items.to(torch.int64))
        r = torch.div(key, int(n_items), rounding_mode="floor")
        noff = torch.zeros(n + 1, dtype=torch.int64, device=off.device)
        noff[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
        return noff, (key - r * int(n_items)).to(torch.int32).contiguous()

    def _sequence_query_tables(self, rows):
        """A temporary table set whose user side is the composed query rows (n, D): the retrieval kernels read nothing
        else of it but the item side, which is the model's."""
        ps = self.net.table_params()
        zero = torch.zeros((rows.shape[0], 1), dtype=torch.float32, device=rows.device)
        return ops.make_tables(rows, ps[1].data, zero, ps[3].data)

    def _sequence_topk(self, rows, k, seen, return_scores, order=None):
        dev = rows.device
        T, keep = self._sequence_query_tables(rows)
        fold = ops.item_fold("linear", T, self.n_items, self.n_factors, dev, None)
        q = torch.arange(rows.shape[0], dtype=torch.int64, device=dev)
        ids, scores, _ = self._chunked(lambda us: ops.retrieve_topk("linear", T, fold, us, k, seen), q)
        ids, scores = ids.cpu(), scores.cpu()
        if order is not None:
            ids, scores = ids[order], scores[order]
        ids = self._original_ids(ids, getattr(self.data_processor, "item_index", None))
        return (ids, scores) if return_scores else ids

    @_host_side
    def recommend_next(self, user_ids, top_k: int = 10, exclude_seen: bool = True, return_scores: bool = False):
        """recommend() under the sequence model: each user's query row is U[u] plus the weighted context rows of the
        LAST items of the user's full train sequence (trs_seq_user_rows), ranked against every item by <q, V[i]> + b[i]
        with recommend()'s fused top-k.  Conventions as recommend(): original ids in and out, (n, k) int64 CPU tensor,
        k = min(top_k, n_items), with return_scores also the (n, k) fp32 scores; exclude_seen drops the user's train
        items; id -1 / score -inf beyond the candidates; ties by ascending item row.  top_k <= TRS_RETRIEVE_KMAX and
        n_factors <= TRS_RETRIEVE_DMAX (ValueError); RuntimeError before fit_sequence().  A user without train rows is
        ranked by U[u] alone.  The sequences are in the model object's order (set_sequence_order()): after
        load_state_dict() that is the input position until the timestamps are given again."""
        what = "recommend_next"
        self._check_sequence_model(what)
        self._check_sequence_topk(what, top_k)
        C, w = self._sequence_buffers(what)
        ulist = user_ids.tolist() if hasattr(user_ids, "tolist") else list(user_ids)
        k = min(int(top_k), self.n_items)
        if k <= 0 or not ulist:
            return self._empty_topk(len(ulist), k, return_scores)
        users = self._dense_users(ulist).to(_device())
        self.net = self.net.eval()
        off, ids = self._sequences()
        err = torch.zeros(1, dtype=torch.int32, device=users.device)
        rows = ops.seq_user_rows(self.net.tables(), C, self._gather_csr(off, ids, users), users, w, err_flag=err)
        seen = self._gather_csr(*self._seen_csr(), users) if exclude_seen else None
        if seen is not None and seen[1].numel() == 0:
            seen = None
        out = self._sequence_topk(rows, k, seen, return_scores)
        check_err_flag(err, what)
        return out

    @_host_side
    def recommend_for_sequences(self, sequences, top_k: int = 10, exclude_seen: bool = True,
                                return_scores: bool = False):
        """recommend_next() for anonymous sessions: `sequences` is a sequence of sequences / 1-D arrays of original item
        ids, oldest first (an unknown id raises IndexError).  The query row is the weighted context rows of the session's
        last items alone (no user row); nothing is fitted.  An empty session ranks by b.  exclude_seen drops the
        session's own items.  Output and limits as recommend_next()."""
        what = "recommend_for_sequences"
        self._check_sequence_model(what)
        self._check_sequence_topk(what, top_k)
        C, w = self._sequence_buffers(what)
        hs = [np.asarray(h.tolist() if hasattr(h, "tolist") else list(h), dtype=np.int64).reshape(-1) for h in sequences]
        n = len(hs)
        lens = np.array([h.size for h in hs], dtype=np.int64)
        flat = np.concatenate(hs) if n and lens.sum() else np.zeros(0, dtype=np.int64)
        dense = self._dense_rows(flat, getattr(self.data_processor, "item_index", None), self.n_items, 'item')
        k = min(int(top_k), self.n_items)
        if k <= 0 or n == 0:
            return self._empty_topk(n, k, return_scores)
        dev = _device()
        self.net = self.net.eval()
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
        ids = dense.to(torch.int32).to(dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        rows = ops.seq_user_rows(self.net.tables(), C, (off, ids), None, w, err_flag=err)
        seen = self._distinct_csr(off, ids, self.n_items) if exclude_seen and ids.numel() else None
        out = self._sequence_topk(rows, k, seen, return_scores)
        check_err_flag(err, what)
        return out

    @_host_side
    def evaluate_next(self, k: int = 10, users=None):
        """Next-item metrics after fit_sequence(holdout_last=True): for every user with a held-out last interaction
        (or those of `users`, original ids), the exact rank (trs_item_ranks; rank_items()'s definition) of the held-out
        item among all items but the user's EARLIER train items, given the context that precedes it.  Returns
        {'hit_rate@k', 'ndcg@k', 'mrr@k'} and the same three for the context-free row U[u] alone under
        '..._no_context', plus 'n_users'; hit = rank < k, ndcg = 1 / log2(rank + 2) and mrr = 1 / (rank + 1) where it
        hits, 0 otherwise, averaged in float64 over the evaluated users."""
        what = "evaluate_next"
        self._check_sequence_model(what)
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"{what}: k must be an integer >= 1, got {k!r}")
        if self.n_factors > ops._lib.RETRIEVE_DMAX:
            raise ValueError(f"{what} takes n_factors <= {ops._lib.RETRIEVE_DMAX} (TRS_RETRIEVE_DMAX), got "
                             f"{self.n_factors}")
        C, w = self._sequence_buffers(what)
        held = getattr(self, "_seq_holdout", None)
        if held is None:
            raise RuntimeError(f"{what}: nothing is held out; call fit_sequence(holdout_last=True) first")
        dense = None if users is None else torch.unique(self._dense_users(users))
        k = int(k)
        dev = _device()
        self.net = self.net.eval()
        off, ids = self._sequences()
        hu, hp = held
        if dense is not None:
            pick = torch.isin(hu, dense.to(dev))
            hu, hp = hu[pick], hp[pick]
        names = [f"{m}@{k}" for m in ("hit_rate", "ndcg", "mrr")]
        out = {name + sfx: 0.0 for sfx in ("", "_no_context") for name in names}
        n = int(hu.numel())
        if n:
            prefix = self._gather_csr(off, ids, hu, drop_last=1)  # what precedes the held-out item
            err = torch.zeros(1, dtype=torch.int32, device=dev)
            rows = ops.seq_user_rows(self.net.tables(), C, prefix, hu, w, err_flag=err)
            seen = self._distinct_csr(*prefix, self.n_items)
            targets = (torch.arange(n + 1, dtype=torch.int64, device=dev), ids[hp].contiguous())
            q = torch.arange(n, dtype=torch.int64, device=dev)
            for sfx, qrows in (("", rows), ("_no_context", self.net.table_params()[0].data[hu].contiguous())):
                T, keep = self._sequence_query_tables(qrows)
                fold = ops.item_fold("linear", T, self.n_items, self.n_factors, dev, None)
                ranks = torch.cat([ops.item_ranks("linear", T, fold, q[s:s + self.RECOMMEND_CHUNK],
                                                  (targets[0][s:s + self.RECOMMEND_CHUNK + 1] - s,
                                                   targets[1][s:s + self.RECOMMEND_CHUNK]), seen)[0]
                                   for s in range(0, n, self.RECOMMEND_CHUNK)]).cpu().numpy().astype(np.float64)
                hit = ranks < k
                out[names[0] + sfx] = float(hit.mean())
                out[names[1] + sfx] = float(np.where(hit, 1.0 / np.log2(ranks + 2.0), 0.0).mean())
                out[names[2] + sfx] = float(np.where(hit, 1.0 / (ranks + 1.0), 0.0).mean())
            check_err_flag(err, what)
        for name, value in out.items():
            print(f'|--- Testing {name}: {value:.4f}')
        out['n_users'] = n
        return out

    # ------------------------------------------------------------------------------------------------ item fold-in
    def _new_item_metadata(self, what, metadata, n):
        """The (n, M) int64 numpy metadata ids of n new items, or None for a model without metadata.  ValueError when
        given without / missing with a metadata model, or of another shape or type; IndexError outside a table."""
        M = self.net.n_meta_tables()
        if M == 0:
            if metadata is not None:
                raise ValueError(f"{what}: metadata given, but the model uses no metadata")
            return None
        if metadata is None:
            raise ValueError(f"{what}: the model uses {M} metadata column(s): metadata (n, {M}) is required")
        meta = np.asarray(metadata.tolist() if hasattr(metadata, "tolist") else metadata)
        if meta.size == 0:
            meta = meta.reshape(-1, M).astype(np.int64)
        if meta.dtype.kind not in 'iu' or meta.shape != (n, M):
            raise ValueError(f"{what}: metadata must be ({n}, {M}) integers, got {meta.dtype} {tuple(meta.shape)}")
        meta = meta.astype(np.int64)
        for m, p in enumerate(self.net.table_params()[4:4 + M]):
            bad = (meta[:, m] < 0) | (meta[:, m] >= p.shape[0])
            if bad.any():
                raise IndexError(f"{what}: metadata id {int(meta[bad, m][0])} of column {m} outside [0, {p.shape[0]})")
        return meta

    def _meta_tables(self):
        """(metadata tables, their 1-wide tables) of the scorer, as make_tables takes them."""
        tp, M = self.net.table_params(), self.net.n_meta_tables()
        return [p.data for p in tp[4:4 + M]], ([p.data for p in tp[4 + M:4 + 2 * M]] if self.net.META_LIN_NAME else [])

    def _new_item_fold(self, meta, n, dev):
        """Item fold of n items whose own rows are zero and whose metadata ids are `meta` (numpy (n, M) or None): its S
        rows are the metadata parts T, its c the constants kappa, of the new items (include/trs.h "item fold-in")."""
        tp = self.net.table_params()
        metas, meta_lins = self._meta_tables()
        zero = torch.zeros((n, self.n_factors), dtype=torch.float32, device=dev)
        zero_lin = torch.zeros((n, 1), dtype=torch.float32, device=dev)
        T, keep = ops.make_tables(tp[0].data, zero, tp[2].data, zero_lin, metas, meta_lins)
        ids = None if meta is None else torch.from_numpy(meta).to(torch.int32).to(dev)
        return ops.item_fold(self.net.NET, T, n, self.n_factors, dev, ids)

    @_host_side
    def fold_in_items(self, histories, metadata=None, epochs: int = 8, lr: float = 0.05, loss: str = 'hinge',
                      l2: float = 0.0, negative_visits: int = 1, seed: int = 0, shuffle: bool = True,
                      reject_seen: bool = True, max_tries: int = 8, return_loss: bool = False):
        """Rows for items the model has never seen, fitted to the users who interacted with them with everything else
        frozen: CPU tensors V (n, n_factors) fp32 and b (n,) fp32 — what the item table and item_bias / linear_item
        would hold — and with return_loss the (epochs, n) fp32 mean pair loss of every epoch.
        histories: a sequence of sequences / 1-D arrays of original user ids (an unknown id raises IndexError); each is
        sorted and de-duplicated first.  metadata: the (n, M) integer metadata ids of the new items, as the ingest took
        them; required exactly when the model uses metadata (ValueError otherwise; IndexError for an id outside its
        table).  The item is scored as item row + metadata rows, so an empty history gives v = 0, b = 0: the item its
        metadata alone describes.
        Per item, `epochs` passes of per-visit SGD over the history (shuffled per epoch when `shuffle`): at each user of
        the history the new item is the positive against one sampled catalogue item (one the user has in the train
        split is redrawn, at most max_tries candidates, when reject_seen); then `negative_visits` (0..8) times the new
        item is the negative of a train interaction drawn uniformly from the train rows this process holds (one whose
        user is in the history is redrawn when reject_seen) — what fit() does to every item through its sampler, and
        what keeps b from growing without bound.  loss 'hinge' or 'bpr' on the scorer's outputs, step lr, L2
        coefficient l2 on v and b; the exact rule is in include/trs.h ("item fold-in").  The result for an item does
        not depend on the other items of the call.  One kernel launch for all items.
        Linear and FM only (ValueError for the MLP and for n_factors > TRS_RETRIEVE_DMAX).  The model's parameters are
        never written; recommend_with_new_items() ranks the catalogue extended by the returned rows."""
        self._check_fold_in("fold_in_items", epochs, lr, loss, l2, seed, max_tries, reject_seen)
        if isinstance(negative_visits, bool) or not isinstance(negative_visits, (int, np.integer)) or \
                not 0 <= int(negative_visits) <= 8:
            raise ValueError(f"negative_visits must be an integer in 0..8, got {negative_visits!r}")
        off, users, rank = self._history_csr(histories, side='user')
        n = rank.size
        meta = self._new_item_metadata("fold_in_items", metadata, n)
        if n == 0:
            V, b = torch.empty((0, self.n_factors), dtype=torch.float32), torch.empty((0,), dtype=torch.float32)
            return (V, b, torch.empty((int(epochs), 0), dtype=torch.float32)) if return_loss else (V, b)
        dev = _device()
        self.net = self.net.eval()
        st = self._device_stream('train')
        if int(negative_visits) > 0 and st['user'].numel() == 0:
            raise ValueError("fold_in_items: negative_visits > 0 needs train interactions, and this process holds none")
        fold = ops.item_fold(self.net.NET, self.net.tables(), self.n_items, self.n_factors, dev, self._item_meta_dev())
        order = np.argsort(rank)  # CSR row k is the caller's item order[k]
        new_fold = self._new_item_fold(None if meta is None else meta[order], n, dev)
        hist = (torch.from_numpy(off).to(dev), torch.from_numpy(users).to(dev))
        V, b, ls = ops.fold_in_items(self.net.NET, self.net.tables(), fold, self.n_items, new_fold, hist, st['user'],
                                     st['pos'], self._seen_csr() if reject_seen else None, loss, int(epochs),
                                     float(lr), float(l2), int(negative_visits), int(seed), bool(shuffle),
                                     bool(reject_seen), int(max_tries), want_loss=return_loss)
        r = torch.from_numpy(rank)
        V, b = V.cpu()[r], b.cpu()[r]
        return (V, b, ls.cpu()[:, r]) if return_loss else (V, b)

    @staticmethod
    def _extended_seen_csr(off, items, hist_off, hist_users, n_items):
        """The seen CSR (numpy offsets (n_users + 1,), items) with row n_items + j appended to the row of every user of
        history j (hist_off, hist_users: a CSR of dense, distinct users per new item).  The new rows are larger than
        every catalogue row and ascend with j, so each user's row stays sorted.  (offsets int64, items int32)."""
        off, items = np.asarray(off, dtype=np.int64), np.asarray(items, dtype=np.int32)
        hist_off, hist_users = np.asarray(hist_off, dtype=np.int64), np.asarray(hist_users, dtype=np.int64)
        n_users = off.size - 1
        rows = np.repeat(np.arange(hist_off.size - 1, dtype=np.int64), np.diff(hist_off)) + int(n_items)
        o = np.lexsort((rows, hist_users))  # by user, then by new row
        au, ar = hist_users[o], rows[o]
        cnt = np.bincount(au, minlength=n_users).astype(np.int64)
        shift = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        new_off = off + shift
        out = np.empty(items.size + ar.size, dtype=np.int32)
        old_user = np.repeat(np.arange(n_users, dtype=np.int64), np.diff(off))
        out[np.arange(items.size, dtype=np.int64) + shift[old_user]] = items
        within = np.arange(ar.size, dtype=np.int64) - shift[au]
        out[new_off[au + 1] - cnt[au] + within] = ar
        return new_off, out

    @_host_side
    def recommend_with_new_items(self, user_ids, item_ids, V, b, metadata=None, histories=None, top_k: int = 10,
                                 exclude_seen: bool = True, return_scores: bool = False):
        """recommend() over the catalogue extended by new items: `item_ids` (original ids, distinct, none of them an item
        of the model: ValueError otherwise) with the rows V (n, n_factors) and 1-wide entries b (n,) that fold_in_items
        returned (or any other), and their (n, M) `metadata` ids exactly when the model uses metadata.
        Output as recommend(): an (n_q, k) int64 CPU tensor of original item ids, k = min(top_k, n_items + n), with
        return_scores also the (n_q, k) fp32 scores (FM: sigmoid(z), ranked by z); positions beyond the candidates hold
        id -1 / score -inf; ties by ascending row, the new items taking the rows after the catalogue's in the order
        given.  exclude_seen drops every user's train items and, with `histories` (one sequence of original user ids
        per new item, as given to fold_in_items), the new item for the users of its history.
        Composition of the existing kernels over temporary tables: the item-side tables are copied with the new rows
        appended, folded (trs_item_fold) and searched (trs_retrieve_topk).  The copy costs one item table per call —
        512 MB at 1 M items x 128 factors — plus its fold; the model is never written or grown.  Only the fused kernel is
        offered: top_k > TRS_RETRIEVE_KMAX raises ValueError, as do the MLP and n_factors > TRS_RETRIEVE_DMAX."""
        what = "recommend_with_new_items"
        self._refuse_ease(f"{what}()", "a new item needs a new fit_ease() over interactions that hold it", ValueError)
        if self.net_type not in ('linear', 'fm'):
            raise ValueError(f"{what} needs net_type 'linear' or 'fm', not {self.net_type!r} (mlp)")
        if self.n_factors > ops._lib.RETRIEVE_DMAX:
            raise ValueError(f"{what} takes n_factors <= {ops._lib.RETRIEVE_DMAX} (TRS_RETRIEVE_DMAX), got "
                             f"{self.n_factors}")
        if int(top_k) > ops._lib.RETRIEVE_KMAX:
            raise ValueError(f"{what} takes top_k <= {ops._lib.RETRIEVE_KMAX} (TRS_RETRIEVE_KMAX), got {top_k}")
        new_ids = np.asarray(item_ids.tolist() if hasattr(item_ids, "tolist") else list(item_ids), dtype=np.int64)
        new_ids = new_ids.reshape(-1)
        n = new_ids.size
        if np.unique(new_ids).size != n:
            raise ValueError(f"{what}: item_ids must be distinct")
        index = getattr(self.data_processor, "item_index", None)
        known = (new_ids >= 0) & (new_ids < self.n_items) if index is None else \
            np.isin(new_ids, index.cpu().numpy().astype(np.int64))
        if known.any():
            raise ValueError(f"{what}: item id {int(new_ids[known][0])} is an item of the model, not a new one")
        V = torch.as_tensor(V, dtype=torch.float32).cpu()
        b = torch.as_tensor(b, dtype=torch.float32).cpu().reshape(-1)
        if tuple(V.shape) != (n, self.n_factors) or b.numel() != n:
            raise ValueError(f"{what}: V must be ({n}, {self.n_factors}) and b ({n},), got {tuple(V.shape)} and "
                             f"{tuple(b.shape)}")
        meta = self._new_item_metadata(what, metadata, n)
        if histories is not None:
            if len(histories) != n:
                raise ValueError(f"{what}: {len(histories)} histories for {n} new items")
            hoff, husers, hrank = self._history_csr(histories, side='user')
        ulist = user_ids.tolist() if hasattr(user_ids, "tolist") else list(user_ids)
        users = self._dense_users(ulist) if ulist else None
        n_all = self.n_items + n
        k = min(int(top_k), n_all)
        if k <= 0 or not ulist:
            return self._empty_topk(len(ulist), k, return_scores)
        dev = _device()
        self.net = self.net.eval()
        tp = self.net.table_params()
        metas, meta_lins = self._meta_tables()
        item = torch.cat([tp[1].data, V.to(dev)])
        item_lin = torch.cat([tp[3].data, b.to(dev).view(-1, 1)])
        T, keep = ops.make_tables(tp[0].data, item, tp[2].data, item_lin, metas, meta_lins)
        item_meta = None if meta is None else \
            torch.cat([self._item_meta_dev(), torch.from_numpy(meta).to(torch.int32).to(dev)]).contiguous()
        fold = ops.item_fold(self.net.NET, T, n_all, self.n_factors, dev, item_meta)
        seen = self._seen_csr() if exclude_seen else None
        if seen is not None and histories is not None and husers.size:
            # the CSR rows are longest first: history row hrank[j] belongs to new item j, catalogue row n_items + j
            off_j = np.concatenate([[0], np.cumsum(np.diff(hoff)[hrank])]).astype(np.int64)
            users_j = np.concatenate([husers[hoff[r]:hoff[r + 1]] for r in hrank])
            eo, ei = self._extended_seen_csr(seen[0].cpu().numpy(), seen[1].cpu().numpy(), off_j, users_j, self.n_items)
            seen = (torch.from_numpy(eo).to(dev), torch.from_numpy(ei).to(dev))
        ids, scores, _ = self._chunked(lambda us: ops.retrieve_topk(self.net.NET, T, fold, us, k, seen),
                                       users.to(dev))
        ids = ids.cpu()
        new = ids >= self.n_items
        new_at = ids[new] - self.n_items
        ids = self._original_ids(torch.where(new, torch.full_like(ids, -1), ids), index)
        ids[new] = torch.from_numpy(new_ids)[new_at]
        return (ids, scores.cpu()) if return_scores else ids

    # ------------------------------------------------------------------------------------------------ neighbours
    def _dense_rows(self, ids, index, n_rows, what):
        """Table rows of a list of caller ids of one side (`what`: 'user' | 'item'); IndexError on an unknown id."""
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
        if index is None:
            bad = (ids < 0) | (ids >= n_rows)
            if bool(bad.any()):
                raise IndexError(f"{what} id {int(ids[bad][0])} outside [0, {n_rows})")
            return ids
        index = index.cpu().to(torch.int64)
        pos = torch.searchsorted(index, ids)
        ok = pos < index.numel()
        ok[ok.clone()] = index[pos[ok]] == ids[ok]
        if not bool(ok.all()):
            raise IndexError(f"{what} id {int(ids[~ok][0])} does not occur in the ingested interactions")
        return pos

    def _similar(self, what, query_ids, top_k, metric, return_scores):
        """similar_items / similar_users: argument checks (before any device work), id mapping, the search, ids back."""
        self._refuse_ease(f"similar_{what}s()", "call item_weights() for an item's strongest weights", ValueError)
        if metric not in ('cosine', 'dot'):
            raise ValueError(f"metric must be 'cosine' or 'dot', got {metric!r}")
        if self.net_type not in ('linear', 'fm'):
            raise ValueError(f"similar_{what}s needs net_type 'linear' or 'fm': with net_type={self.net_type!r} the "
                             "metadata embeddings are concatenated, not summed, so an item has no folded row")
        if self.n_factors > ops._lib.RETRIEVE_DMAX:
            raise ValueError(f"similar_{what}s takes n_factors <= {ops._lib.RETRIEVE_DMAX} (TRS_RETRIEVE_DMAX), got "
                             f"{self.n_factors}")
        self.net = self.net.eval()
        n_rows = self.n_items if what == 'item' else self.n_users
        index = getattr(self.data_processor, f"{what}_index", None)
        qlist = query_ids.tolist() if hasattr(query_ids, "tolist") else list(query_ids)
        k = min(int(top_k), n_rows)
        if k <= 0 or not qlist:
            return self._empty_topk(len(qlist), k, return_scores)
        queries = self._dense_rows(qlist, index, n_rows, what).to(_device())
        ids, scores = self._neighbours_dense(what, queries, k, metric == 'cosine')
        ids = self._original_ids(ids.cpu(), index)
        return (ids, scores.cpu()) if return_scores else ids

    def _neighbours_dense(self, what, queries, k, cosine):
        """Top-k neighbours of dense rows (int64 GPU tensor) of the item or the user side: (ids (n, k) dense int64 with
        -1 padding, similarities (n, k) fp32 with -inf padding).  k <= KMAX: the fused kernel over the normalised
        buffer; larger k: rows of a Linear scorer over it, the query's own column -> -inf, trs_topk."""
        dev = queries.device
        D = self.n_factors
        n = queries.numel()
        if what == 'user':
            n_rows, rows = self.n_users, self.net.user.weight.data
        elif self.net.n_meta_tables() == 0:  # S_i is the item row itself
            n_rows, rows = self.n_items, self.net.item.weight.data
        else:
            n_rows = self.n_items
            rows = ops.fold_rows(ops.item_fold(self.net.NET, self.net.tables(), n_rows, D, dev, self._item_meta_dev()),
                                 n_rows)
        nf = ops.neighbour_fold(rows, n_rows, D, cosine)
        if k <= ops._lib.RETRIEVE_KMAX:
            return self._chunked(lambda qs: ops.neighbours_topk(nf, n_rows, D, qs, k), queries)
        X, zero = ops.fold_views(nf, n_rows, D)
        ids = torch.empty((n, k), dtype=torch.int64, device=dev)
        scores = torch.empty((n, k), dtype=torch.float32, device=dev)
        for s in range(0, n, self.GENERIC_CHUNK):
            qs = queries[s:s + self.GENERIC_CHUNK]
            g = qs.numel()
            Tz, keep = ops.make_tables(X[qs].contiguous(), X, zero[:g].view(-1, 1), zero.view(-1, 1))
            sims = torch.stack([ops.score_all_items("linear", Tz, r, n_rows, dev) for r in range(g)])
            sims[torch.arange(g, device=dev), qs] = float('-inf')
            ids[s:s + g], scores[s:s + g] = self._topk_rows(sims, sims, k, torch.full((g,), n_rows - 1, device=dev))
        return ids, scores

    @_host_side
    def similar_items(self, item_ids, top_k: int = 10, metric: str = 'cosine', return_scores: bool = False):
        """The top_k items most similar to each of several items: an (n, k) int64 CPU tensor of original item ids,
        k = min(top_k, n_items); with return_scores also the (n, k) fp32 similarities.
        An item is represented by S_i = item_i + sum_m meta_m(i), the row the scorers multiply with a user's (two items
        with the same metadata and close id rows are close); bias and linear terms take no part.  metric='dot':
        <S_q, S_j>; metric='cosine': the rows are scaled to unit length first (fp32), then the same inner product; a zero
        row is similar to nothing (0 everywhere).  The query's own id is never returned; another item with identical
        values is.  Order: similarity descending, ties by ascending item row as in predict(); the positions beyond the
        n_items - 1 other items hold id -1 and similarity -inf.  An unknown id raises IndexError.
        Linear and FM only (ValueError for the MLP, whose metadata embeddings are concatenated, and for n_factors >
        TRS_RETRIEVE_DMAX).  k <= TRS_RETRIEVE_KMAX runs the fused matrix-core kernel of recommend() on a normalised
        copy of the folded item matrix, built per call; larger k scores rows one query at a time.  Under
        torch.distributed every rank answers from its own replica."""
        return self._similar('item', item_ids, top_k, metric, return_scores)

    @_host_side
    def similar_users(self, user_ids, top_k: int = 10, metric: str = 'cosine', return_scores: bool = False):
        """similar_items() for users: a user is its row of the user table (user_bias / linear_user take no part); the
        result holds original user ids, k = min(top_k, n_users).
        Every call builds a padded (for cosine: unit-length) copy of the user table — n_users rounded up to 128 rows x
        n_factors rounded up to 16/32/64/128/256 columns x 4 bytes, plus 4 bytes per row — which lives for the call:
        5 GB for 10 M users at 128 factors."""
        return self._similar('user', user_ids, top_k, metric, return_scores)

    # ------------------------------------------------------------------------------------------------ diversity
    def _diverse_dense(self, users, k, pool, lam, cosine, exclude_seen, want_ild=False):
        """MMR lists of dense users (int64 GPU tensor, not empty): the fused top-`pool` over one item fold, one neighbour
        fold of the item side (the rows _neighbours_dense uses), trs_mmr_rerank per RECOMMEND_CHUNK.  (ids (n, k) dense
        int64 with -1 padding, scores (n, k) fp32, per-list intra-list diversity on the cosine fold (n,) float64 or None)."""
        dev = users.device
        D = self.n_factors
        fold = ops.item_fold(self.net.NET, self.net.tables(), self.n_items, D, dev, self._item_meta_dev())
        pids, pscores, _ = self._rank_dense(users, pool, exclude_seen, fold=fold)
        rows = self.net.item.weight.data if self.net.n_meta_tables() == 0 else ops.fold_rows(fold, self.n_items)
        nf = ops.neighbour_fold(rows, self.n_items, D, cosine)
        step = self.RECOMMEND_CHUNK
        outs = [ops.mmr_rerank(nf, self.n_items, D, pids[s:s + step], pscores[s:s + step], k, lam)
                for s in range(0, users.numel(), step)]
        ids, scores = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        ild = None
        if want_ild:
            nc = nf if cosine else ops.neighbour_fold(rows, self.n_items, D, True)
            ild = torch.cat([ops.list_ild(nc, self.n_items, D, ids[s:s + step]) for s in range(0, users.numel(), step)])
        return ids, scores, ild

    @_host_side
    def recommend_diverse(self, user_ids, top_k: int = 10, diversity: float = 0.3, pool=None, metric: str = 'cosine',
                          exclude_seen: bool = True, return_scores: bool = False):
        """recommend() with redundancy traded against relevance inside each list: greedy Maximal-Marginal-Relevance
        (MMR) selection of top_k items out of each user's `pool` best ones.  Same conventions as recommend(): original
        ids in and out, an (n, k) int64 CPU tensor, k = min(top_k, n_items), id -1 / score -inf where a user has fewer
        candidates; with return_scores also the picked items' own (n, k) fp32 scores, in pick order.
        The first pick is the user's best item; every further pick maximises
            (1 - diversity) * rel_j  -  diversity * max over the picked s of sim(j, s)
        with rel the pool's scores scaled to [0, 1] per user and sim the cosine (metric='cosine') or inner product
        ('dot') of the items' folded rows S_i = item_i + sum_m meta_m(i), the rows similar_items() compares; ties go to
        the better-ranked item.  diversity=0 returns recommend()'s list, diversity=1 ignores relevance after the first
        pick.  The rule, operation by operation, is in include/trs.h "diversified re-ranking".
        pool defaults to min(TRS_RETRIEVE_KMAX, max(4 top_k, 32), n_items); the fused top-k caps it at
        TRS_RETRIEVE_KMAX = 128.  ValueError: the MLP (no folded rows), n_factors > TRS_RETRIEVE_DMAX, top_k > pool,
        pool > TRS_RETRIEVE_KMAX, a diversity outside [0, 1], an unknown metric.  Per call one item fold, one
        normalised copy of it and one selection launch per 65 536 users; under torch.distributed every rank answers
        from its own replica."""
        self._refuse_ease("recommend_diverse()", "call recommend()", ValueError)
        k, pool = diversity_eval.check('recommend_diverse', self.net_type, self.n_factors, self.n_items, top_k,
                                       diversity, pool, metric, ops._lib.RETRIEVE_KMAX, ops._lib.RETRIEVE_DMAX)
        self.net = self.net.eval()
        ulist = user_ids.tolist() if hasattr(user_ids, "tolist") else list(user_ids)
        if k <= 0 or not ulist:
            return self._empty_topk(len(ulist), k, return_scores)
        users = self._dense_users(ulist).to(_device())
        ids, scores, _ = self._diverse_dense(users, k, pool, float(diversity), metric == 'cosine', exclude_seen)
        ids = self._original_ids(ids.cpu(), getattr(self.data_processor, "item_index", None))
        return (ids, scores.cpu()) if return_scores else ids

    def _relevance_csr(self, exclude_seen):
        """CSR of the test split's distinct (user, item) pairs over dense users; with exclude_seen without the pairs
        that are also in the train split (this rank's train rows: under dp_partition 'user' all rows of its users)."""
        dev = _device()
        td = self.data_processor.test_data
        key = torch.unique(td['user_id'].to(torch.int64).to(dev) * int(self.n_items) + td['pos_item_id'].to(torch.int64).to(dev))
        if exclude_seen:
            off, items = self._seen_csr()
            su = torch.repeat_interleave(torch.arange(self.n_users, device=dev), off[1:] - off[:-1])
            key = key[~torch.isin(key, su * int(self.n_items) + items.long())]
        u = torch.div(key, int(self.n_items), rounding_mode="floor")
        off = torch.zeros(self.n_users + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(torch.bincount(u, minlength=self.n_users), 0)
        return off, (key - u * int(self.n_items)).to(torch.int32).contiguous()

    @_host_side
    def evaluate_ranking(self, k: int = 10, metrics=('hit_rate', 'recall', 'ndcg'), exclude_seen: bool = True,
                         users=None):
        """Ranking metrics of recommend() over the full catalogue against the test split; returns
        {f'{m}@{k}': float, 'n_users': int} and prints them as evaluate() does.
        Users: the distinct users of the test split (or `users`, caller ids).  T_u = the user's distinct test items,
        without the ones it also has in train when exclude_seen; users with an empty T_u are skipped.  R_u = the top-k list:
          hit_rate@k = 1[|R_u & T_u| >= 1]     recall@k = |R_u & T_u| / |T_u|
          ndcg@k     = sum_{r<k, R_u[r] in T_u} 1/log2(r+2)  /  sum_{r<min(k,|T_u|)} 1/log2(r+2)
        averaged over the evaluated users (per-user values from the device, sums in float64 in ascending user order).
        Data parallel: rank r evaluates the users with user_id % world == r and the sums are all-reduced (needs
        dp_partition='user' without pre_sharded: a rank must hold all train rows of its users)."""
        unknown = set(metrics) - {'hit_rate', 'recall', 'ndcg'}
        if unknown:
            raise ValueError(f"unknown ranking metrics {sorted(unknown)}")
        rank, world = tdist.world_info()
        if world > 1 and (getattr(self, 'pre_sharded', False) or self.dp_partition != 'user'):
            raise ValueError("evaluate_ranking under data parallelism needs dp_partition='user' without pre_sharded: "
                             "a rank must hold every train and test row of the users it evaluates")
        self.net = self.net.eval()
        dev = _device()
        kk = min(int(k), self.n_items)
        rel = self._relevance_csr(exclude_seen)
        if users is None:
            dense = torch.unique(self.data_processor.test_data['user_id'].to(torch.int64))
        else:
            dense = torch.unique(self._dense_users(users))
        if world > 1:
            dense = dense[dense % world == rank]
        dense = dense.to(dev)
        dense = dense[(rel[0][dense + 1] - rel[0][dense]) > 0]
        sums = np.zeros(4)
        if dense.numel() and kk > 0:
            _, _, met = self._rank_dense(dense, kk, exclude_seen, rel)
            m = met.cpu().numpy()
            sums = np.array([float(np.sum(m[:, 0] >= 1)), float(np.sum(m[:, 0] / m[:, 3])),
                             float(np.sum(m[:, 1] / m[:, 2])), float(m.shape[0])])
        if world > 1:
            sums = np.array(tdist.allreduce_scalar_sum(sums.tolist(), dev))
        n = int(sums[3])
        col = {'hit_rate': 0, 'recall': 1, 'ndcg': 2}
        results = {}
        for metric in metrics:
            value = float(sums[col[metric]] / n) if n else 0.0
            results[f'{metric}@{k}'] = value
            print(f'|--- Testing {metric}@{k}: {value:.4f}')
        results['n_users'] = n
        return results

    @_host_side
    def evaluate_diversity(self, k: int = 10, diversity: float = 0.0, pool=None, metric: str = 'cosine',
                           exclude_seen: bool = True, users=None):
        """Beyond-accuracy metrics of the lists of recommend_diverse(top_k=k, diversity=..., pool=..., metric=...) next
        to their accuracy, for the users evaluate_ranking() evaluates (selected the same way); returns {'ild@k',
        'coverage@k', 'novelty@k', 'hit_rate@k', 'recall@k', 'ndcg@k', 'n_users'} and prints them as evaluate_ranking()
        does.  diversity=0 evaluates plain recommend().
          ild@k      mean over users of the mean of 1 - cosine over the pairs of the list's items (always the cosine of
                     the folded item rows, whatever `metric` the selection used); 0 for a list with fewer than two items
          coverage@k |union of the returned items| / n_items
          novelty@k  mean over users of the mean over the list's items of -log2((c_i + 1) / (n_users + 1)), c_i = the
                     distinct train users of item i
          hit_rate@k, recall@k, ndcg@k   evaluate_ranking()'s formulas on the re-ranked lists
        Per-user values in float64, averaged over the evaluated users in ascending user order (evaluate/diversity.py).
        Under torch.distributed with more than one rank: ValueError (coverage needs the union over all ranks)."""
        self._refuse_ease("evaluate_diversity()", "call evaluate_ranking() or evaluate_ranks()", ValueError)
        kk, pool = diversity_eval.check('evaluate_diversity', self.net_type, self.n_factors, self.n_items, k,
                                        diversity, pool, metric, ops._lib.RETRIEVE_KMAX, ops._lib.RETRIEVE_DMAX)
        rank, world = tdist.world_info()
        if world > 1:
            raise ValueError("evaluate_diversity does not run under data parallelism: coverage@k is the union of the "
                             "lists over all ranks; evaluate on one rank")
        self.net = self.net.eval()
        dev = _device()
        rel = self._relevance_csr(exclude_seen)
        if users is None:
            dense = torch.unique(self.data_processor.test_data['user_id'].to(torch.int64))
        else:
            dense = torch.unique(self._dense_users(users))
        dense = dense.to(dev)
        dense = dense[(rel[0][dense + 1] - rel[0][dense]) > 0]
        names = ('ild', 'coverage', 'novelty', 'hit_rate', 'recall', 'ndcg')
        values = dict.fromkeys(names, 0.0)
        n = 0
        if dense.numel() and kk > 0:
            ids, _, ild = self._diverse_dense(dense, kk, pool, float(diversity), metric == 'cosine', exclude_seen,
                                              want_ild=True)
            m = ops.rank_metrics(ids, dense, rel).cpu().numpy()
            n = m.shape[0]
            item_users = torch.bincount(self._seen_csr()[1].long(), minlength=self.n_items).cpu().numpy()
            lists = ids.cpu().numpy()
            values = {'ild': float(np.sum(ild.cpu().numpy())) / n,
                      'coverage': diversity_eval.coverage(lists, self.n_items),
                      'novelty': float(np.sum(diversity_eval.novelty_per_user(lists, item_users, self.n_users))) / n,
                      'hit_rate': float(np.sum(m[:, 0] >= 1)) / n,
                      'recall': float(np.sum(m[:, 0] / m[:, 3])) / n,
                      'ndcg': float(np.sum(m[:, 1] / m[:, 2])) / n}
        results = {}
        for name in names:
            results[f'{name}@{k}'] = values[name]
            print(f'|--- Testing {name}@{k}: {values[name]:.4f}')
        results['n_users'] = n
        return results


class FitRunner:
    """One training run at a fixed batch size: owns the optimiser plan, the staging buffers and the per-epoch batch
    feed.  begin_epoch() -> run_steps(k) (any number of calls) -> end_epoch()."""

    def __init__(self, model, optimizer, batch_size):
        self.m = model
        self.batch_size = batch_size
        self.dev = _device()
        self.data = model._rank_rows(model.data_processor.train_data)
        self.sampler = model._sampler() if model.rng == 'device' else None
        # k negatives per positive: the epoch visits every training row k times (k * N positions)
        self.n_train = self.data['user_id'].shape[0] * (self.sampler.k if self.sampler else 1)
        self.loader = FastDataLoader(data=self.data, batch_size=batch_size, shuffle=True,
                                     dynamic_neg_sampling=model.dynamic_neg_sampling, n_items=model.n_items,
                                     item_to_metadata_map=model.data_processor.item_meta_table,
                                     metadata_id_cols=model.metadata_name) if model.rng == 'reference' else None
        self.num_batches = int(math.ceil(self.n_train / batch_size)) if self.n_train > 0 else 0
        self.own_batches = self.num_batches
        if model.net_type == 'mlp' and tdist.world_info()[1] > 1:
            # the MLP all-reduces its dense gradients every step: all ranks run the common (minimum) number of steps per
            # epoch; the shard stays whole, so the positions beyond are other rows every epoch (the epoch shuffle)
            import torch.distributed as _d
            dev = self.dev if _d.get_backend() == 'nccl' else torch.device('cpu')
            self.num_batches = tdist.allreduce_min_int(self.num_batches, dev)
            if self.num_batches < self.own_batches:
                print(f'|--- data parallel: rank {tdist.world_info()[0]} runs {self.num_batches} of its '
                      f'{self.own_batches} steps per epoch (about '
                      f'{self.n_train - min(self.n_train, self.num_batches * batch_size)} of {self.n_train} positions '
                      'wait for another epoch\'s shuffle)')
        self.trainer = model._make_trainer(optimizer, min(batch_size, max(self.n_train, 1)))
        if getattr(self.trainer, "M", 0) > 0:
            self.trainer.item_meta = model._item_meta_dev()  # metadata scorers: the presort groups each column too
        self.trainer.sampler = self.sampler
        self.loss_sums = torch.zeros(max(self.num_batches, 1), dtype=torch.float32, device=self.dev)
        self.next_batch = 0
        self.ep = None
        self._next_ep = None
        self.prep_out = None
        # MLP (fused embedding update, device RNG): ids AND duplicate flags of 256 batches at a time from the sparse
        # regime's presort (trs_epoch_flags: the same triples trs_batch_prepare generates) instead of a prepare launch
        # per step — with the flags, the update's rows that are alone in their batch (94-97 % at c5) take plain
        # read-modify-writes instead of float atomics.  TRS_MLP_SLICE_FLAGS=0: a prepare launch per step, all atomics.
        self._mlp_ef, self._mlp_slice = None, None
        if (model.rng == 'device' and type(self.trainer).__name__ == "MLPTrainer" and
                getattr(self.trainer, "kind", None) == "sgd" and self.trainer._fused_embed_lr() is not None and
                batch_size <= ops.EpochFlags.MAX_BATCH and os.environ.get("TRS_MLP_SLICE_FLAGS", "1") != "0" and
                self.dev.type == "cuda" and self.n_train >= batch_size):
            self._mlp_ef = ops.EpochFlags(min(256, self.n_train // batch_size), batch_size, model.n_users,
                                          model.n_items, self.dev, ordered=False)

    def begin_epoch(self):
        m = self.m
        self.loss_sums.zero_()
        self.next_batch = 0
        self._slice = None
        self._epoch_no = getattr(self, "_epoch_no", 0) + 1
        if self.num_batches == 0:
            return
        if m.rng == 'reference':
            if self._next_ep is not None:  # drawn by prepare_next_epoch() while the previous epoch's steps ran
                self.ep, self._next_ep = self._next_ep, None
            else:
                iter(self.loader)  # reshuffle: one torch.randperm per epoch (dataset.py:369-373)
                self.ep = m._host_epoch(self.data, self.loader)
        else:
            self.st = m._device_stream('train')
            self.shuffle_key, self.sample_seed = self._epoch_keys(m._fit_epochs_done)

    def prepare_next_epoch(self):
        """Reference-RNG mode: draw the NEXT epoch's batches (shuffle + sampler, in the reference's RNG order — nothing
        else consumes the generators in between) right after the current epoch's steps were enqueued, so the host work
        overlaps the GPU instead of following the epoch's loss read-back.  Only fit() calls this, and only when another
        epoch follows: the generators are left exactly where the reference leaves them."""
        if self.m.rng == 'reference' and self.num_batches > 0 and self._next_ep is None:
            iter(self.loader)
            self._next_ep = self.m._host_epoch(self.data, self.loader)

    def _epoch_keys(self, epochs_done):
        """(shuffle key, sampler seed) of the device-RNG epoch that follows `epochs_done` finished ones."""
        seed = self.m.seed + 1000003 * tdist.world_info()[0]  # every rank draws its own negatives
        return _mix64(seed, 2 * epochs_done + 1), _mix64(seed, 2 * epochs_done + 2)

    def _presort(self, s0, full, prefetch=False, next_epoch=False):
        m, B, sl = self.m, self.batch_size, self.trainer.SLICE_BATCHES
        nb = min(sl, full - s0)
        tag = (self._epoch_no + int(next_epoch), s0, nb, B)
        if m.rng == 'device':
            sk, ss = self._epoch_keys(m._fit_epochs_done + 1) if next_epoch else (self.shuffle_key, self.sample_seed)
            return self.trainer.presort_slice(nb, B, self.st, sk, ss, s0 * B, tag=tag, prefetch=prefetch)
        assert not next_epoch  # the reference-RNG epoch is drawn from the host generators at begin_epoch
        return self.trainer.presort_slice(nb, B, given_ids=[self.ep[k_][s0 * B:(s0 + nb) * B]
                                                            for k_ in ('user', 'pos', 'neg')], tag=tag,
                                          prefetch=prefetch)

    def run_steps(self, k):
        """Run the next k steps of the current epoch (stops at the epoch's end).  Returns the number of steps run."""
        m, B = self.m, self.batch_size
        done = 0
        kind = getattr(self.trainer, "fast_kind", None)
        # the C step loop: SGD on every path, SparseAdam / Adagrad on the presorted path only
        has_meta = getattr(self.trainer, "M", 0) > 0  # metadata scorers: presorted path only (SGD)
        if os.environ.get("TRS_META_FAST", "1") == "0" and has_meta:
            kind = None  # tuning / fall-back knob: metadata scorers on the generic staged path
        fast = (kind == "sgd" and not has_meta) or (kind is not None and self.trainer.wants_presort(B))
        # losses and regularisers that stage their gradients step by step (engine.SparseScorerTrainer.per_step_only):
        # the per-step loop below, on K candidates per row where the loss trains on them
        per_step = self.trainer.per_step_only()
        n_cand = self.trainer.n_candidates() if per_step else None
        # score-aware mining: the negative of step t depends on the tables after step t - 1, so neither the slice-ahead
        # presort nor the C step loop applies — the per-step loop below, one mining launch in front of every step
        mining = getattr(self.sampler, "mine", None) is not None
        fast = fast and not per_step and not mining
        if fast and m.rng == 'reference':
            fast = self.ep['user'].dtype == torch.int32
        ops.stamp("run_steps:setup")
        if fast:  # whole batches, step loop in C (csrc/fast_step.hip): from the resident stream, or from the epoch's
            full = self.n_train // B  # host-prepared id arrays (bit-exact reference batches)
            presort = self.trainer.wants_presort(B)
            while done < k and self.next_batch < full:
                n = min(k - done, full - self.next_batch, 64)
                b = self.next_batch
                if presort:  # item references grouped by row per slice of batches (csrc/presort.hip)
                    sl = self.trainer.SLICE_BATCHES
                    if self._slice is None or not (self._slice[0] <= b < self._slice[0] + self._slice[1].n_batches):
                        s0 = (b // sl) * sl
                        self._slice = (s0, self._presort(s0, full))
                        if s0 + sl < full:  # next slice: sorted on a side stream while this slice's steps run
                            self._presort(s0 + sl, full, prefetch=True)
                        elif m.rng == 'device' and getattr(self, 'more_epochs', True):  # last slice: the next epoch's keys
                            # are known, start on its first slice
                            self._presort(0, full, prefetch=True, next_epoch=True)
                    s0, ps = self._slice
                    n = min(n, s0 + ps.n_batches - b)
                    ops.stamp("run_steps:before_fast_sorted_steps")
                    self.trainer.fast_sorted_steps(ps, b - s0, B, n, self.loss_sums[b:b + n],
                                                   m._item_meta_dev() if has_meta else None)
                elif m.rng == 'device' and self.sampler is None:
                    self.trainer.fast_stream_steps(self.st, self.shuffle_key, self.sample_seed, b * B, B, n,
                                                   self.loss_sums[b:b + n])
                elif m.rng == 'device':  # sampler options live in the presort / batch_prepare generators
                    break
                else:
                    self.trainer.fast_array_steps(self.ep, b * B, B, n, self.loss_sums[b:b + n])
                self.next_batch += n
                done += n
        while done < k and self.next_batch < self.num_batches:
            b = self.next_batch
            s, e = b * B, min((b + 1) * B, self.n_train)
            if m.rng == 'reference':
                ids = {key: v[s:e] for key, v in self.ep.items()}
            elif self._mlp_ef is not None and e - s == B:
                ids = self._mlp_slice_ids(b)
            else:
                st = self.st
                out = self.prep_out if (self.prep_out is not None and e - s == B) else None
                if n_cand is not None:
                    ids = ops.batch_prepare_multi(st['user'], st['pos'], self.shuffle_key, s, e - s, m.n_items,
                                                  self.sample_seed, s, n_cand, st['item_meta'], out,
                                                  sampler=self.sampler)
                elif mining:  # K candidates scored under the tables as step b - 1 left them, one launch on this stream
                    ids = ops.batch_prepare_mined(st['user'], st['pos'], self.shuffle_key, s, e - s, m.n_items,
                                                  self.sample_seed, s, m.net.NET, m.net.tables(), self.sampler,
                                                  st['item_meta'], out)
                else:
                    ids = ops.batch_prepare(st['user'], st['pos'], st['neg'], self.shuffle_key, s, e - s, m.n_items,
                                            self.sample_seed, s, st['item_meta'], out, sampler=self.sampler)
                if e - s == B:
                    self.prep_out = ids
            self.trainer.loss_step(ids, self.loss_sums[b:b + 1])
            self.next_batch += 1
            done += 1
        return done

    def _mlp_slice_ids(self, b):
        """ids + duplicate flags of whole batch b as views of the current 256-batch slice (generated on the launch
        stream when the epoch enters the slice: 0.8 ms per 256 steps of >= 1.5 ms each)."""
        ef, B, st = self._mlp_ef, self.batch_size, self.st
        cur = self._mlp_slice
        if cur is None or cur[0] != self._epoch_no or not (cur[1] <= b < cur[1] + cur[2]):
            s0 = (b // ef.n_batches) * ef.n_batches
            nb = min(ef.n_batches, self.n_train // B - s0)
            if "ui" not in st:
                st["ui"] = ops.interleave_stream(st["user"], st["pos"])
            ef.run(st["ui"], st["neg"], self.shuffle_key, self.sample_seed, s0 * B, self.trainer.err,
                   sampler=self.sampler, n_batches=nb)  # (the epoch's last slice may be shorter)
            meta = None
            if st.get("item_meta") is not None:
                n = nb * B
                meta = (st["item_meta"][ef.ids[1][:n].long()], st["item_meta"][ef.ids[2][:n].long()])
            cur = self._mlp_slice = (self._epoch_no, s0, nb, meta)
        o = (b - cur[1]) * B
        ids = {"user": ef.ids[0][o:o + B], "pos": ef.ids[1][o:o + B], "neg": ef.ids[2][o:o + B],
               "user_dup": ef.user_dup[o:o + B], "item_dup": ef.item_dup[o:o + B]}
        if cur[3] is not None:
            ids["pos_meta"], ids["neg_meta"] = cur[3][0][o:o + B], cur[3][1][o:o + B]
        return ids

    def touch_host_path(self):
        """Walk the host side of the next run_steps() call with ZERO steps: the same Python code and the same C entry
        point, no kernel launch and no state change (the C step loop with n_steps = 0 returns at once; a pending slice
        switch is left to the real call).  For callers that time a SHORT window right after a synchronise (bench.py with
        the driver's 20 steps): the thread wakes from the wait with cold caches and its first pass through this code
        takes ~75 us instead of ~12 (host time stamps, TRS_BENCH_TIMELINE=1) — 9 % of such a window, nothing in a
        training run of thousands of steps.  Returns True if the path was walked."""
        m, B = self.m, self.batch_size
        tr = self.trainer
        if getattr(tr, "fast_kind", None) != "sgd" or getattr(tr, "M", 0) > 0 or not tr.wants_presort(B):
            return False
        b = self.next_batch
        if self._slice is None or not (self._slice[0] <= b < self._slice[0] + self._slice[1].n_batches):
            return False
        s0, ps = self._slice
        tr.fast_sorted_steps(ps, b - s0, B, 0, self.loss_sums[b:b + 1])  # (zero steps: the slot is not written)
        return True

    def end_epoch(self):
        """Sync once, check the id-range flag, return the reference's epoch loss (unweighted mean of batch means)."""
        m, B = self.m, self.batch_size
        m._fit_epochs_done += 1
        sums = self.loss_sums.cpu().numpy()
        self.trainer.check_errors()
        total = 0.0
        for b in range(self.next_batch):
            nb = min((b + 1) * B, self.n_train) - b * B
            total += float(np.float32(sums[b]) / np.float32(nb))
        return total / self.next_batch if self.next_batch > 0 else 0
