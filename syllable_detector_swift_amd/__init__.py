"""syllable_detector_swift_amd -- MI355X-native batched syllable detection.

One hot path of gardner-lab/syllable-detector-swift (STFT -> band slice -> sliding window
-> feed-forward net -> threshold) as hand-written HIP kernels for gfx950 behind the C ABI
in include/syldet.h.  Importing this package loads libsyldet.so and fails if it has not
been built: there is no CPU implementation in the product.
"""
from . import _abi
from .config import (InvalidValue, MismatchedLength, MissingValue, NeuralNet, NeuralNetLayer, ParseError,
                     ProcessingFunction, SyllableDetectorConfig, SyllableDetectorError, UnableToOpenPath,
                     createWindow, frequencyIndexRange)
from .bank import PinnedArray, ShardedSyllableDetectorBank, shard_table
from ._abi import ALIGN_COLUMNS, ALIGN_OUTPUTS, ALIGN_SAMPLES, PCM_F32, PCM_F64, PCM_S16, PCM_S24, PCM_S32, PCM_U8
from .detector import (PCM24, Aligner, Matcher, MatcherBank, matchClassesHost, matchNormalizeHost, matchPeaksHost, matchScoresHost, Recordings, Scorer, SyllableDetector, Trainer, MultiTrainer, trainParamCount, trainTargetsHost, trainAdamHost, trainInitHost, trainInputMapHost, alignHost, alignStatsHost, chooseThreshold, configsCompatible, configsShareClock, fusedFormOfConfig,
                       pcmDecode, pcmSampleBytes, planRecordings, recordingLengths, scoreHost)
from .resampler import ResamplerLinear, ResamplerSinc, sincReady, convertRate, deinterleave, sincCoefficient, sincDefaults, sincTaps

__all__ = ["SyllableDetector", "SyllableDetectorConfig", "NeuralNet", "NeuralNetLayer", "ProcessingFunction",
           "ParseError", "UnableToOpenPath", "MissingValue", "InvalidValue", "MismatchedLength",
           "SyllableDetectorError", "frequencyIndexRange", "createWindow", "ResamplerLinear", "deinterleave",
           "convertRate", "ResamplerSinc", "sincReady", "sincCoefficient", "sincTaps", "sincDefaults",
           "ShardedSyllableDetectorBank", "PinnedArray", "shard_table", "configsCompatible",
           "configsShareClock", "fusedFormOfConfig", "Recordings", "planRecordings", "recordingLengths", "Scorer", "scoreHost", "chooseThreshold",
           "PCM_U8", "PCM_S16", "PCM_S24", "PCM_S32", "PCM_F32", "PCM_F64", "PCM24", "pcmDecode", "pcmSampleBytes",
           "Aligner", "alignHost", "alignStatsHost", "ALIGN_COLUMNS", "ALIGN_OUTPUTS", "ALIGN_SAMPLES",
           "Trainer", "MultiTrainer", "trainParamCount", "trainTargetsHost", "trainAdamHost", "trainInitHost", "trainInputMapHost",
           "Matcher", "matchNormalizeHost", "matchScoresHost", "matchPeaksHost",
           "MatcherBank", "matchClassesHost"]
