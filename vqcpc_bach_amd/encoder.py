"""Encoder composition and the trainer base class (reference: VQCPCB/encoder.py:12-110, 216-325)."""
import os

import torch
from torch import nn

from . import ops
from .training import FlatTraining, checkpoint_dir
from .utils import flatten


class Encoder(nn.Module):
    """data_processor -> downscaler -> quantizer -> upscaler  (encoder.py:31-45, 76-95)."""

    def __init__(self, model_dir, data_processor, downscaler, quantizer, upscaler):
        super().__init__()
        self.data_processor = data_processor
        self.downscaler = downscaler
        self.quantizer = quantizer
        self.upscaler = upscaler
        self.model_dir = model_dir

    # ---- checkpoints: one torch.save(state_dict) per sub-module, reference file names (encoder.py:47-74) --------
    def _dir(self, early_stopped):
        return checkpoint_dir(self.model_dir, early_stopped)

    def save(self, early_stopped):
        model_dir = self._dir(early_stopped)
        os.makedirs(model_dir, exist_ok=True)
        torch.save(self.data_processor.state_dict(), f'{model_dir}/data_processor')
        torch.save(self.downscaler.state_dict(), f'{model_dir}/downscaler')
        torch.save(self.quantizer.state_dict(), f'{model_dir}/quantizer')
        if self.upscaler is not None:
            torch.save(self.upscaler.state_dict(), f'{model_dir}/upscaler')

    def load(self, early_stopped, device):
        print(f'Loading models {self.__repr__()}')
        model_dir = self._dir(early_stopped)
        if not os.path.exists(model_dir):      # older layout
            model_dir = self.model_dir
        ml = torch.device(device)
        self.data_processor.load_state_dict(torch.load(f'{model_dir}/data_processor', map_location=ml))
        self.downscaler.load_state_dict(torch.load(f'{model_dir}/downscaler', map_location=ml))
        self.quantizer.load_state_dict(torch.load(f'{model_dir}/quantizer', map_location=ml))
        if self.upscaler:
            self.upscaler.load_state_dict(torch.load(f'{model_dir}/upscaler', map_location=ml))
        # loaded codebooks must never be overwritten by the data-dependent initialisation of the first batch
        # (main_encoder.py:51 builds the quantizer with initialize = not load for the same reason)
        if hasattr(self.quantizer, 'initialize'):
            self.quantizer.initialize = False

    # ---- forward ---------------------------------------------------------------------------------------------
    def encode_many(self, xs, corrupt_flags=None, with_loss_rows=False):
        """Encode several token tensors (batch_i, ticks_i, voices) in ONE pass: all 16-token blocks are independent
        (relative_transformer_downscaler.py:98-115), so the calls of vqcpc_encoder_trainer.py:201-231 merge into one
        launch sequence.  The FIRST tensor plays the role of the reference's first call for the data-dependent
        codebook initialisation.  Returns a list of (z_quantized, encoding_indices, quantization_loss)."""
        corrupt_flags = corrupt_flags or [False] * len(xs)
        tpb = self.downscaler.sequence_length
        toks = [self.data_processor.preprocess(x) for x in xs]               # (batch_i, nb_i, 16)
        # BachDataProcessor (student configuration) keeps (batch, events, voices): cut it into blocks of `tpb` tokens,
        # token p of a block = (event p // voices, voice p % voices), i.e. utils.flatten + the view of
        # relative_transformer_downscaler_linear.py:104-107
        toks = [t if t.shape[-1] == tpb else t.reshape(t.shape[0], -1, tpb) for t in toks]
        sizes = [t.shape[0] * t.shape[1] for t in toks]
        tokens = torch.cat([t.reshape(-1, tpb) for t in toks], dim=0) if len(toks) > 1 else toks[0].reshape(-1, tpb)
        tokens = self.data_processor.checked(tokens)
        z = self.downscaler.forward_tokens(tokens.unsqueeze(0), self.data_processor)[0]        # (R, D)
        starts = [sum(sizes[:i]) for i in range(len(sizes))]
        corrupt_rows = None
        if any(corrupt_flags):
            corrupt_rows = torch.cat([torch.arange(s, s + n, device=z.device)
                                      for s, n, f in zip(starts, sizes, corrupt_flags) if f])
        zq, idx, ql = self.quantizer(z, corrupt_labels=any(corrupt_flags), init_rows=slice(0, sizes[0]),
                                     corrupt_rows=corrupt_rows)
        if self.upscaler is not None:
            zq = self.upscaler(zq)
        out = []
        zq_parts = ops.SplitRowsFn.apply(zq, *sizes) if (len(sizes) > 1 and zq.requires_grad) else None
        for i, (t, s, n) in enumerate(zip(toks, starts, sizes)):
            b, nb = t.shape[0], t.shape[1]
            idx_i = idx[s:s + n].view(b, nb, -1) if idx is not None else None
            zq_i = zq_parts[i] if zq_parts is not None else zq[s:s + n]
            out.append((zq_i.view(b, nb, -1), idx_i, ql[s:s + n].view(b, nb)))
        # with_loss_rows: also the quantisation loss of ALL rows of the pass (the trainer's q-loss sums every segment)
        return (out, ql) if with_loss_rows else out

    def forward(self, x, corrupt_labels=False):
        """x (batch, num_ticks, num_voices) ints from the dataloader ->
        z_quantized (batch, nb, z_dim), encoding_indices (batch, nb, num_codebooks), quantization_loss (batch, nb)."""
        return self.encode_many([x], [corrupt_labels])[0]

    def forward_embedded(self, x_embed, corrupt_labels=False):
        """API-compatible tail of the reference forward for callers that already hold embeddings (encoder.py:84-95)."""
        z = self.downscaler.forward(flatten(x_embed))
        zq, idx, ql = self.quantizer(z, corrupt_labels=corrupt_labels)
        if self.upscaler is not None:
            zq = self.upscaler(zq)
        return zq, idx, ql

    @torch.no_grad()
    def encode_indices(self, x, merged=False):
        """Inference path (what decoders/decoder.py:327-336 and the cluster tools encoder.py:137-159 consume): token
        tensor (batch, ticks, voices) -> encoding_indices (batch, nb, num_codebooks) int64 [or merged codes
        (batch, nb)], without materialising the straight-through output, the loss or the upscaler.  Uses the modules'
        current train/eval mode for dropout like `forward` does; call `.eval()` first for deterministic codes."""
        tpb = self.downscaler.sequence_length
        t = self.data_processor.preprocess(x)
        t = t if t.shape[-1] == tpb else t.reshape(t.shape[0], -1, tpb)
        t = self.data_processor.checked(t)
        z = self.downscaler.forward_tokens(t.unsqueeze(0), self.data_processor)[0]             # (batch, nb, D)
        q = self.quantizer
        assert not q.initialize, 'the codebooks are still waiting for their data-dependent initialisation'
        from . import ops
        idx = ops.vq_assign(z.reshape(-1, z.shape[-1]), torch.stack(list(q.embeddings), dim=0))
        idx = idx.view(z.shape[0], z.shape[1], -1)
        return self.merge_codes(idx) if merged else idx

    @torch.no_grad()
    def encode_latents(self, x):
        """The latents a decoder on continuous sources consumes (decoders/decoder.py:327-336 with a NoQuantization
        quantizer): token tensor (batch, ticks, voices) -> z (batch, nb, D) float32, the downscaler's output; no quantizer, no
        upscaler.  Inference only, in eval mode (the caller's train / eval state is put back)."""
        was_training = self.training
        self.eval()
        try:
            tpb = self.downscaler.sequence_length
            t = self.data_processor.preprocess(x)
            t = t if t.shape[-1] == tpb else t.reshape(t.shape[0], -1, tpb)
            t = self.data_processor.checked(t)
            z = self.downscaler.forward_tokens(t.unsqueeze(0), self.data_processor)[0]         # (batch, nb, D)
        finally:
            self.train(was_training)
        return z.detach().to(torch.float32).contiguous()

    def quantizer_needs_init(self):
        """True while the codebooks still wait for their data-dependent initialisation (first training batch)."""
        return bool(getattr(self.quantizer, 'initialize', False))

    def merge_codes(self, codes):
        """sum_c codes[..., c] * codebook_size**c  (encoder.py:97-110, without its aliasing `+=`)."""
        ret = codes[..., 0].clone()
        for c in range(1, codes.shape[-1]):
            ret = ret + codes[..., c] * (self.quantizer.codebook_size ** c)
        return ret

    # ---- "Explore clusters" (main_encoder.py:100-118; encoder.py:112-200) ----------------------------------------------------------
    def plot_clusters(self, dataloader_generator, split_name, batch_size=32, num_batches=64):
        """What the codes of `split_name` stand for (encoder.py:112-176): the cluster census (clusters.cluster_census) of the
        generator's corpus, written as `{model_dir}/clusters_{split_name}.npz` (ClusterCensus.save) and
        `{model_dir}/clusters_{split_name}.txt` (its tables, every codebook), and returned.  The WHOLE split is visited:
        `batch_size` and `num_batches` are accepted for the reference's signature and ignored.  Needs a corpus generator (one with
        `device_corpus`): the synthetic generators have no corpus to show."""
        from . import clusters
        if split_name not in ('train', 'val', 'test'):
            raise ValueError(f'{split_name} is not a valid split value. Choose between train, val or test')
        dc = getattr(dataloader_generator, 'device_corpus', None)
        if dc is None:
            raise NotImplementedError('plot_clusters shows blocks of a corpus: it needs a corpus dataloader generator '
                                      '(dataloaders/corpus.py), not a synthetic one')
        census = clusters.cluster_census(self, dc, split=split_name)
        os.makedirs(self.model_dir, exist_ok=True)
        census.save(f'{self.model_dir}/clusters_{split_name}.npz')
        with open(f'{self.model_dir}/clusters_{split_name}.txt', 'w') as f:
            f.write('\n'.join(census.table(codebook=c) for c in range(census.num_codebooks)))
        return census

    def show_nn_clusters(self, k=3):
        """Prints, per codeword of codebook 0, its k nearest other codewords (encoder.py:178-185, same lines), then the further
        codebooks under a header line each; returns the (num_codebooks, codebook_size, k) int32 array.  Neighbours are ordered by
        (squared distance, index) and a codeword is left out of its own list by index (vqcpc_codebook_knn)."""
        from . import clusters
        if not hasattr(self.quantizer, 'embeddings'):
            raise ValueError(f'show_nn_clusters: a {type(self.quantizer).__name__} encoder has no codebook')
        nn_idx, _ = clusters.codebook_knn(torch.stack([e.detach() for e in self.quantizer.embeddings], dim=0), k)
        nn_idx = nn_idx.cpu().numpy()
        for c, book in enumerate(nn_idx):
            print('Nearest neighbours list:' if c == 0 else f'Nearest neighbours list (codebook {c}):')
            for i, res in enumerate(book):
                print(f'{i}: {res}')
        return nn_idx

    def scatterplot_clusters_3d(self):
        raise NotImplementedError('the 3-d scatter plot of a codebook of dimension 3 needs matplotlib: out of scope '
                                  '(SURVEY.md section 2, #4)')


class EncoderTrainer(FlatTraining, nn.Module):
    """Epoch loop, checkpoints, logging (encoder.py:216-325); the step protocol is training.FlatTraining's."""

    def __init__(self, dataloader_generator):
        super().__init__()
        self.dataloader_generator = dataloader_generator
        self.writer = None

    def to(self, device):
        for m in self._modules_with_params():
            m.to(device)
        return self

    def train(self, mode=True):
        for m in self._modules_with_params():
            m.train(mode)
        return self

    def eval(self):
        return self.train(False)

    def _checkpoint_owners(self):
        return [self, self.encoder]             # `save` writes the encoder's files through encoder.save

    def train_model(self, batch_size, num_batches, num_epochs, lr, corrupt_labels, schedule_lr, plot=False, num_workers=0,
                    weight_average=None, **kwargs):
        if plot:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.writer = SummaryWriter(f'{self.model_dir}')
            except Exception:                  # tensorboard is optional (not installed in the ROCm image)
                self.writer = None
        with self._training_defaults():
            self.init_optimizers(lr=lr, schedule_lr=schedule_lr)
            if weight_average is not None:
                self.enable_weight_averaging(weight_average)
            return self._train_epochs(batch_size, num_batches, num_epochs, num_workers, monitor='loss_monitor',
                                      save_best=lambda: self.save(early_stopped=True),
                                      save_every=lambda: self.save(early_stopped=False),
                                      after_epoch=self.plot if plot and self.writer is not None else None,
                                      corrupt_labels=corrupt_labels)

    def plot(self, epoch_id, monitored_quantities_train, monitored_quantities_val, index_encoder=None):
        suffix = f'_{index_encoder})' if index_encoder is not None else ''
        for tag, quantities in (('train', monitored_quantities_train), ('val', monitored_quantities_val)):
            if quantities is None:
                continue
            for k, v in quantities.items():
                if isinstance(v, list):
                    for ind, elem in enumerate(v):
                        self.writer.add_scalar(f'{k}_{ind}{suffix}/{tag}', elem, epoch_id)
                else:
                    self.writer.add_scalar(f'{k}{suffix}/{tag}', v, epoch_id)
