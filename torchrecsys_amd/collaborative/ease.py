# -*- coding: utf-8 -*-
"""EASE (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019; reference collaborative/ease.py): an
item-item model with a closed form.  The net has no parameters: its one tensor is the (n_items, n_items) fp32 weight
matrix B that TorchRecSys.fit_ease() computes (include/trs.h "EASE"), kept as a persistent buffer so that state_dict()
carries it.  A user's score row is the sum of the B rows of the user's train items (trs_ease_scores)."""
import torch

from .. import ops

_UNFITTED = "call fit_ease() first"


class EASE(torch.nn.Module):
    def __init__(self, n_users, n_items, **_ignored):
        super().__init__()
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.register_buffer("B", None)  # (n_items, n_items) fp32 once fitted
        self._hist = None         # (offsets int64 (n_users + 1,), items int32) GPU CSR of the train split
        self._hist_source = None  # callable that builds it (a model restored by load_state_dict was never fitted)

    def bind_history(self, source):
        """source() -> the train split's seen CSR; called at most once, when a score is first asked for."""
        object.__setattr__(self, "_hist_source", source)

    def set_weights(self, B, hist):
        """What fit_ease() hands over: B (n_items, n_items) fp32 on the GPU and the seen CSR it was fitted on."""
        if tuple(B.shape) != (self.n_items, self.n_items) or B.dtype != torch.float32:
            raise ValueError(f"B must be ({self.n_items}, {self.n_items}) fp32, got {tuple(B.shape)} {B.dtype}")
        self.B = B.contiguous()
        object.__setattr__(self, "_hist", hist)

    def weights(self):
        if self.B is None:
            raise RuntimeError(_UNFITTED)
        return self.B

    def history(self):
        if self._hist is None:
            if self._hist_source is None:
                raise RuntimeError(_UNFITTED)
            object.__setattr__(self, "_hist", self._hist_source())
        return self._hist

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        B = state_dict.get(prefix + "B")
        if B is not None and self.B is None:  # a fresh model takes the fitted one's weights
            if tuple(B.shape) != (self.n_items, self.n_items):
                error_msgs.append(f"size mismatch for {prefix}B: {tuple(B.shape)} for a catalogue of {self.n_items} items")
                return
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else B.device
            self.B = torch.empty((self.n_items, self.n_items), dtype=torch.float32, device=dev)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    # -------------------------------------------------------------------------------------------- inference
    def score_rows(self, users):
        """Score rows (len(users), n_items) fp32 of dense users (int64 GPU tensor) in one launch."""
        B = self.weights()
        return ops.ease_scores(B, self.history(), users.to(torch.int64).contiguous())

    def score_all_items(self, user_id, item_meta_dev=None):
        """Scores of one user against every item, (n_items,) fp32 on the GPU: predict()."""
        B = self.weights()
        if not 0 <= user_id < self.n_users:
            raise IndexError(f"index out of range in self (user_id {user_id} outside [0, {self.n_users}))")
        return self.score_rows(torch.tensor([int(user_id)], dtype=torch.int64, device=B.device))[0]
