# -*- coding: utf-8 -*-
"""Item kNN: the sparse item-item neighbourhood model (co-occurrence similarities, K neighbours kept per item; Sarwar
et al., WWW 2001, Deshpande & Karypis, TOIS 2004).  The net has no parameters: its tensors are the neighbour lists that
TorchRecSys.fit_itemknn() computes (include/trs.h "item kNN"), nbr_ids (n_items, K) int32 and nbr_w (n_items, K) fp32,
and a three-entry float64 record of how they were made (similarity kind, shrinkage, K), kept as persistent buffers so
that state_dict() carries them.  A user's score row is the sum, over the user's train items, of the weights their lists
give each column (trs_knn_scores).  The model is n_items x K entries, so it takes catalogues EASE cannot."""
import torch

from .. import ops

_UNFITTED = "call fit_itemknn() first"


class ItemKNN(torch.nn.Module):
    def __init__(self, n_users, n_items, **_ignored):
        super().__init__()
        self.n_users, self.n_items = int(n_users), int(n_items)
        self.register_buffer("nbr_ids", None)  # (n_items, K) int32 once fitted, -1 beyond a row's candidates
        self.register_buffer("nbr_w", None)    # (n_items, K) fp32, 0 there
        self.register_buffer("knn_meta", None)  # (3,) float64: TRS_KNN_* kind, shrinkage, K
        self._hist = None         # (offsets int64 (n_users + 1,), items int32) GPU CSR of the train split
        self._hist_source = None  # callable that builds it (a model restored by load_state_dict was never fitted)

    def bind_history(self, source):
        """source() -> the train split's seen CSR; called at most once, when a score is first asked for."""
        object.__setattr__(self, "_hist_source", source)

    def set_neighbours(self, ids, w, hist, kind, shrinkage):
        """What fit_itemknn() hands over: the lists (n_items, K) int32 / fp32 on the GPU, the seen CSR they were built
        on, and the similarity (TRS_KNN_* id) and shrinkage that made them.  A row lists a column at most once."""
        if ids.dim() != 2 or ids.shape[0] != self.n_items or ids.shape != w.shape or ids.dtype != torch.int32 or \
                w.dtype != torch.float32 or not 1 <= ids.shape[1] <= ops._lib.KNN_KMAX:
            raise ValueError(f"nbr_ids / nbr_w must be ({self.n_items}, K) int32 / fp32 with K in 1.."
                             f"{ops._lib.KNN_KMAX}, got {tuple(ids.shape)} {ids.dtype} / {tuple(w.shape)} {w.dtype}")
        self.nbr_ids, self.nbr_w = ids.contiguous(), w.contiguous()
        self.knn_meta = torch.tensor([float(kind), float(shrinkage), float(ids.shape[1])], dtype=torch.float64,
                                     device=ids.device)
        object.__setattr__(self, "_hist", hist)

    def neighbours(self):
        if self.nbr_ids is None:
            raise RuntimeError(_UNFITTED)
        return self.nbr_ids, self.nbr_w

    def history(self):
        if self._hist is None:
            if self._hist_source is None:
                raise RuntimeError(_UNFITTED)
            object.__setattr__(self, "_hist", self._hist_source())
        return self._hist

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        ids, w = state_dict.get(prefix + "nbr_ids"), state_dict.get(prefix + "nbr_w")
        if ids is not None and w is not None and self.nbr_ids is None:  # a fresh model takes the fitted one's lists
            if ids.dim() != 2 or ids.shape[0] != self.n_items or ids.shape != w.shape:
                error_msgs.append(f"size mismatch for {prefix}nbr_ids / {prefix}nbr_w: {tuple(ids.shape)} / "
                                  f"{tuple(w.shape)} for a catalogue of {self.n_items} items")
                return
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else ids.device
            self.nbr_ids = torch.empty(tuple(ids.shape), dtype=torch.int32, device=dev)
            self.nbr_w = torch.empty(tuple(ids.shape), dtype=torch.float32, device=dev)
            self.knn_meta = torch.empty(3, dtype=torch.float64, device=dev)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    # -------------------------------------------------------------------------------------------- inference
    def score_csr_rows(self, hist, rows):
        """Score rows (len(rows), n_items) fp32 of the rows `rows` (int64 GPU tensor) of any history CSR."""
        ids, w = self.neighbours()
        return ops.knn_scores(ids, w, hist, rows.to(torch.int64).contiguous())

    def score_rows(self, users):
        """Score rows (len(users), n_items) fp32 of dense users (int64 GPU tensor) in one launch."""
        self.neighbours()
        return self.score_csr_rows(self.history(), users)

    def score_all_items(self, user_id, item_meta_dev=None):
        """Scores of one user against every item, (n_items,) fp32 on the GPU: predict()."""
        ids, _ = self.neighbours()
        if not 0 <= user_id < self.n_users:
            raise IndexError(f"index out of range in self (user_id {user_id} outside [0, {self.n_users}))")
        return self.score_rows(torch.tensor([int(user_id)], dtype=torch.int64, device=ids.device))[0]
