"""MI355X-native FastSpeech2 mel-generation forward pass.

``FeedForwardTransformer`` is a drop-in for the reference's ``fastspeech.FeedForwardTransformer``
(reference fastspeech.py:28); its arithmetic runs in ``libfs2_hip.so`` (C ABI: include/fs2.h).
"""
from .hparams import default_hparams, load_hparams, N_PHONEME_SYMBOLS  # noqa: F401
from .fastspeech import FeedForwardTransformer, StepStreams  # noqa: F401
from .io import load_checkpoint, vocoder_input, hparams_from_str  # noqa: F401
from .vocoder import GriffinLim, Geometry, Waveforms, AsyncWaveforms, mel_basis, mel_energy, pitch, wav_features, stft_magnitude, save_wav, spsi_phase  # noqa: F401
from .vocoder import PitchTrack, pitch_candidates, pitch_path, pitch_track  # noqa: F401
from .vocoder import f0_phase, excitation  # noqa: F401
from .targets import TargetStats, TrainingTargets, clean_targets, hp_data, remove_outlier, training_targets  # noqa: F401
from .losses import LossTerms, loss_terms  # noqa: F401
from .dtw import DtwTerms, mel_dtw  # noqa: F401
from .align import Alignment, monotonic_align  # noqa: F401
from .prosody import ProsodyPrediction, label_means, semitones  # noqa: F401
