"""Allowed-token masks for template-based generation (`Decoder.generate_from_codes(allowed=...)` and the long forms): host
helpers that turn a corpus's token names (`DeviceCorpus.names` / `load_corpus(...).names`, the `index2note_dicts` of the
reference's dataset) into bool masks (..., events, voices, vmax).  No kernel here: the sampler applies the packed masks.

    kinds = token_kinds(corpus.names, corpus.vocab)                       # (voices, vmax) int16
    g_major = torch.zeros(events, 12, dtype=torch.bool)
    g_major[:, [7, 9, 11, 0, 2, 4, 6]] = True
    allowed = rhythm_mask(chorale, kinds) & pitch_class_mask(kinds, g_major) & range_mask(kinds, low, high)

Masks combine with `&`; a combination that leaves some (event, voice) without a token is refused by the generation call,
which names the place.  Rules BETWEEN the voices -- no crossing, bounded leaps, no parallel fifths or octaves -- are not masks:
`VoiceLeadingRules` (`rules=`) is applied on the device during the generation (csrc/rules.hip)."""
import re

import numpy as np
import torch

HOLD, REST, META = -1, -2, -3
_STEPS = {'C': 0, 'D': 2, 'E': 4, 'F': 5, 'G': 7, 'A': 9, 'B': 11}
_NOTE = re.compile(r'^([A-Ga-g])(#*|-*)(\d+)$')          # music21's nameWithOctave: letter, sharps or flats, octave


def _kind(name):
    if name == '__':
        return HOLD
    if name == 'rest':
        return REST
    m = _NOTE.match(name)
    if m is None:
        return META                                        # START, END, XX, '' and anything else
    step, acc, octave = m.groups()
    midi = 12 * (int(octave) + 1) + _STEPS[step.upper()] + (len(acc) if acc.startswith('#') else -len(acc))
    return midi if 0 <= midi <= 127 else META


def token_kinds(names, vocab):
    """names (voices, vmax) strings, vocab the voices' vocabulary sizes -> (voices, vmax) int16: the MIDI pitch of a note name
    ('C4' -> 60, 'B-3' -> 58, 'F##2' -> 43), HOLD for '__', REST for 'rest', META for START / END / XX / '' / anything
    unparsable and for every index at or past the voice's vocabulary."""
    names = np.asarray(names).astype(str)
    vocab = [int(v) for v in vocab]
    if names.ndim != 2 or names.shape[0] != len(vocab) or names.shape[1] < max(vocab):
        raise ValueError(f'token_kinds: names (voices, >= max vocab) and one vocabulary size per voice expected, got '
                         f'{names.shape} and {len(vocab)} sizes')
    out = torch.full(names.shape, META, dtype=torch.int16)
    for c, v in enumerate(vocab):
        for i in range(v):
            out[c, i] = _kind(str(names[c, i]))
    return out


def _kinds(kinds):
    kinds = torch.as_tensor(kinds)
    if kinds.dim() != 2 or kinds.is_floating_point():
        raise ValueError(f'kinds: the (voices, vmax) integer table of token_kinds expected, got {tuple(kinds.shape)}')
    return kinds.cpu().long()


class VoiceLeadingRules:
    """Relational rules between the voices, for `generate_from_codes(rules=...)` and the long forms.  Unlike the masks above
    they cannot be decided before the generation: whether a token breaks one depends on what the other voices drew at this
    tick and on the pitch every voice still holds, so a kernel (csrc/rules.hip) narrows every position's token set on the
    device, between two steps, from the tokens emitted so far.

        rules = VoiceLeadingRules(kinds, no_crossing=True, max_leap=12, no_parallels=True)

    kinds: the (voices, vmax) table of `token_kinds`.  The voices are ordered top to bottom by index -- soprano = 0, as in the
    Bach corpus; another order is not supported.
    no_crossing: a voice never sounds above a voice of lower index or below one of higher index.
    max_leap: None (off), one int >= 0 for every voice, or one entry per voice (None or negative: off for that voice): the
    largest step in semitones from the pitch the voice sounded last (through holds; a rest forgets it).
    no_parallels: no parallel fifths or octaves (unisons included) between two voices that move in the same direction.
    A voice is compared with the voices already drawn at its tick and with those a `constraint` forces.  Where the rules leave
    no token of the position's set, they are relaxed for that position -- parallels first, then the leap, then the crossing --
    and `return_rule_report=True` says where: bit 0 CROSSING, bit 1 LEAP, bit 2 PARALLEL were dropped; a forced token reports
    the rules it breaks in bits 4..6.  ValueError on a wrong table, a negative max_leap, or when no rule is enabled."""
    CROSSING, LEAP, PARALLEL = 1, 2, 4

    def __init__(self, kinds, no_crossing=True, max_leap=None, no_parallels=False):
        kinds = torch.as_tensor(kinds)
        if kinds.dim() != 2 or kinds.is_floating_point() or kinds.is_complex() or kinds.dtype == torch.bool or \
                not 1 <= kinds.shape[0] <= 16 or not 1 <= kinds.shape[1] <= 256:
            raise ValueError(f'VoiceLeadingRules: the (voices <= 16, vmax <= 256) integer table of token_kinds expected, got '
                             f'{tuple(kinds.shape)} {kinds.dtype}')
        kinds = kinds.cpu().to(torch.int64)
        if bool((kinds < META).any()) or bool((kinds > 127).any()):
            raise ValueError('VoiceLeadingRules: kinds holds MIDI pitches in [0, 127], HOLD, REST or META')
        voices = kinds.shape[0]
        if max_leap is None:
            leaps = [-1] * voices
        elif isinstance(max_leap, (int, np.integer)) and not isinstance(max_leap, bool):
            if max_leap < 0:
                raise ValueError(f'VoiceLeadingRules: max_leap >= 0 expected, got {max_leap}')
            leaps = [int(max_leap)] * voices
        else:
            try:
                leaps = [-1 if m is None or int(m) < 0 else int(m) for m in max_leap]
            except TypeError:
                raise ValueError(f'VoiceLeadingRules: max_leap is None, an int or one entry per voice, got {max_leap!r}')
            if len(leaps) != voices:
                raise ValueError(f'VoiceLeadingRules: one max_leap per voice ({voices}) expected, got {len(leaps)}')
        self.kinds = kinds.to(torch.int32).contiguous()
        self.max_leap = torch.tensor(leaps, dtype=torch.int32)
        self.no_crossing, self.no_parallels = bool(no_crossing), bool(no_parallels)
        self.mask = (self.CROSSING if self.no_crossing else 0) | (self.LEAP if any(m >= 0 for m in leaps) else 0) | \
            (self.PARALLEL if self.no_parallels else 0)
        if self.mask == 0:
            raise ValueError('VoiceLeadingRules: no rule is enabled')


def rhythm_mask(template_tokens, kinds):
    """template_tokens (..., events, voices) int64, kinds from `token_kinds` -> bool (..., events, voices, vmax) that keeps the
    template's rhythm: where it holds only HOLD is allowed, where it starts a note any pitched token, where it rests only
    REST, where it has a meta symbol everything."""
    kinds = _kinds(kinds)
    nc, vmax = kinds.shape
    tok = torch.as_tensor(template_tokens).cpu().long()
    if tok.dim() < 2 or tok.shape[-1] != nc or bool((tok < 0).any()) or bool((tok >= vmax).any()):
        raise ValueError(f'rhythm_mask: tokens (..., events, {nc}) in [0, {vmax}) expected, got {tuple(tok.shape)}')
    k = kinds[torch.arange(nc), tok]                                             # the template token's kind, (..., events, voices)
    k = k.unsqueeze(-1)
    pitched = kinds >= 0
    return torch.where(k >= 0, pitched, torch.where(k == META, torch.ones_like(pitched), kinds == k))


def pitch_class_mask(kinds, pitch_classes):
    """pitch_classes (events, 12) bool, the pitch classes (0 = C) open at every event -> bool (events, voices, vmax): a pitched
    token is allowed where its pitch class is; HOLD and REST always; META never."""
    kinds = _kinds(kinds)
    pcs = torch.as_tensor(pitch_classes)
    if pcs.dim() != 2 or pcs.shape[1] != 12 or pcs.dtype != torch.bool:
        raise ValueError(f'pitch_class_mask: (events, 12) bool expected, got {tuple(pcs.shape)} {pcs.dtype}')
    inside = pcs.cpu()[:, kinds.clamp(min=0) % 12]                                 # (events, voices, vmax)
    return torch.where(kinds >= 0, inside, ((kinds == HOLD) | (kinds == REST)).expand_as(inside))


def range_mask(kinds, low, high):
    """low, high: one MIDI bound per voice (inclusive) -> bool (1, voices, vmax), which broadcasts over the events of the
    masks it is combined with: a pitched token is allowed inside its voice's range; HOLD and REST always; META never."""
    kinds = _kinds(kinds)
    low, high = torch.as_tensor(low).long().reshape(-1, 1), torch.as_tensor(high).long().reshape(-1, 1)
    if low.shape[0] != kinds.shape[0] or high.shape[0] != kinds.shape[0]:
        raise ValueError(f'range_mask: one low and one high bound per voice ({kinds.shape[0]}) expected')
    return (((kinds >= low) & (kinds <= high)) | (kinds == HOLD) | (kinds == REST)).unsqueeze(0)
