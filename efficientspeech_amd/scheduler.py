"""Length-bucketed batching of ragged inference requests.

The reference pads a batch to its longest utterance and -- a quirk kept on purpose -- lets padded key
positions take part in attention, so every padded phoneme is pure waste on the device AND changes the numbers of the
utterances it is batched with.  `BucketedSynthesizer` sorts requests by length and cuts them into batches of at most
`max_batch` utterances whose lengths fall into one bucket of `granularity` phonemes: granularity 1 never pads (only
equal-length utterances share a batch), a larger one trades a bounded amount of padding (< granularity phonemes per
utterance) for fuller batches.  Each batch is one `Phoneme2Mel` forward; results come back in request order.

With a `vocoder` (the HIP `hifigan.Generator`) each batch also goes through the length-aware generator -- `mel_len` handed over on
the device, no work for the frames behind an utterance's end in the stages of at most 64 channels -- and every request gets its waveform trimmed to `mel_len * hop`.
"""
import numpy as np
import torch

from .networks import CONTROL_KEYS, get_mask_from_lengths


class BucketedSynthesizer:
    def __init__(self, net, max_batch=256, granularity=8, pad_id=0, vocoder=None):
        assert max_batch >= 1 and granularity >= 1
        self.net, self.max_batch, self.granularity, self.pad_id = net, int(max_batch), int(granularity), int(pad_id)
        self.vocoder = vocoder

    def plan(self, lengths):
        """-> list of (request indices, padded length T) covering every request once, longest bucket first."""
        lengths = np.asarray(lengths, dtype=np.int64)
        order = np.argsort(-lengths, kind="stable")
        g = self.granularity
        batches, cur, cur_bucket = [], [], None
        for i in order:
            bucket = (int(lengths[i]) + g - 1) // g
            if cur and (bucket != cur_bucket or len(cur) == self.max_batch):
                batches.append((cur, int(lengths[cur[0]])))
                cur = []
            cur.append(int(i))
            cur_bucket = bucket
        if cur:
            batches.append((cur, int(lengths[cur[0]])))
        return batches

    @staticmethod
    def padding_waste(lengths, batches):
        """fraction of phoneme slots that are padding under `batches`"""
        lengths = np.asarray(lengths, dtype=np.int64)
        slots = sum(len(idx) * T for idx, T in batches)
        return 1.0 - float(lengths.sum()) / max(slots, 1)

    @staticmethod
    def _batch_control(v, idx, lengths, T):
        """One key's control of a batch: (B,) when every request of the batch carries a number, else the (B, T) curve -- each request's
        curve (or its number over its row) in the batch's order, 1.0 behind its end."""
        if isinstance(v, np.ndarray):
            return torch.from_numpy(v[idx])
        if all(v[i].ndim == 0 for i in idx):
            return torch.from_numpy(np.array([v[i] for i in idx], np.float32))
        curve = np.ones((len(idx), T), np.float32)
        for r, i in enumerate(idx):
            curve[r, :lengths[i]] = v[i]
        return torch.from_numpy(curve)

    @torch.no_grad()
    def __call__(self, sequences, extra=None, controls=None):
        """sequences: list of 1-D integer phoneme id sequences.  -> list (request order) of (mel (L_i, n_mel), duration (T_i,)), or
        with a vocoder of (wav (L_i * hop,), mel (L_i, n_mel), duration (T_i,)).
        `extra(indices, T)` may return additional input-dict entries for a batch (e.g. forced durations).
        `controls`: per-REQUEST prosody scales, a dict with any of `pitch_control`, `energy_control`, `duration_control`, each an array
        of len(sequences) numbers; every batch gets its requests' entries (unrelated requests share a batch, each keeps its own scale).
        A request's entry may instead be a per-phoneme curve: a 1-D array of that request's own length (then pass a list, one entry per
        request).  A batch that holds a curve for a key gets a (B, T) tensor for it -- the requests' curves gathered in batch order,
        a number filling its request's row, 1.0 behind each request's end; a batch of numbers only keeps the (B,) form."""
        dev = self.net.decoder.mel_linear.weight.device
        lengths = [int(len(s)) for s in sequences]
        controls = dict(controls or {})
        for k, v in controls.items():
            if k not in CONTROL_KEYS:
                raise ValueError(f"controls: unknown key {k!r} (one of {', '.join(CONTROL_KEYS)})")
            if torch.is_tensor(v):
                v = v.detach().cpu().numpy()
            if isinstance(v, (list, tuple)) and any(np.ndim(e.detach().cpu() if torch.is_tensor(e) else e) > 0 for e in v):
                if len(v) != len(sequences):
                    raise ValueError(f"controls[{k!r}]: {len(v)} entries, expected one per request ({len(sequences)})")
                per = [np.asarray(e.detach().cpu() if torch.is_tensor(e) else e, dtype=np.float32) for e in v]
                for i, e in enumerate(per):
                    if e.ndim > 0 and e.shape != (lengths[i],):
                        raise ValueError(f"controls[{k!r}][{i}]: shape {e.shape}, expected a number or a curve of the request's length "
                                         f"({lengths[i]},)")
                controls[k] = per
                continue
            controls[k] = np.asarray(v, dtype=np.float32)
            if controls[k].shape != (len(sequences),):
                raise ValueError(f"controls[{k!r}]: shape {controls[k].shape}, expected one scale per request ({len(sequences)},)")
        out = [None] * len(sequences)
        for idx, T in self.plan(lengths):
            ids = np.full((len(idx), T), self.pad_id, np.int32)
            for r, i in enumerate(idx):
                ids[r, :lengths[i]] = np.asarray(sequences[i], dtype=np.int32)
            x = {"phoneme": torch.from_numpy(ids).to(dev)}
            if len(idx) > 1:                                   # the reference's B == 1 path takes no mask (networks.py:338)
                x["phoneme_mask"] = get_mask_from_lengths(torch.tensor([lengths[i] for i in idx], device=dev), T)
            if extra is not None:
                x.update(extra(idx, T))
            for k, v in controls.items():                      # this batch's requests, in the batch's order
                x[k] = self._batch_control(v, idx, lengths, T).to(dev)
            mel, mel_len, dur = self.net(x)
            wav = None
            if self.vocoder is not None and mel.shape[1] > 0:      # (launched before the lengths are read back)
                wav = self.vocoder(mel.transpose(1, 2), lengths=mel_len)[:, 0]
            ml = mel_len.cpu().numpy()
            for r, i in enumerate(idx):
                out[i] = (mel[r, :int(ml[r])], dur[r, :lengths[i], 0])
                if self.vocoder is not None:
                    hop = self.vocoder.h.hop
                    out[i] = ((wav[r, :int(ml[r]) * hop] if wav is not None else mel.new_zeros((0,))),) + out[i]
        return out
