//  Resampler.swift -- replacement for Common/Resampler.swift's ResamplerLinear over libsyldet
//  (bound through the bridging header, see INTEGRATION.md).  Same protocol, same class name and
//  members, so Processor.swift:116-121 and ViewControllerProcessor.swift:247-250 compile unchanged.
//  Not compiled in this repository (no Swift toolchain in the build image).

import Foundation

protocol Resampler {
    func resampleVector(_ data: UnsafePointer<Float>, ofLength numSamples: Int) -> [Float]
}

/// Linear interpolation on the GPU, bit-identical to the original's vDSP_vramp / vDSP_vlint sequence.
class ResamplerLinear: Resampler {
    let samplingRateIn: Double
    let samplingRateOut: Double
    private var handle: OpaquePointer?

    init(fromRate samplingRateIn: Double, toRate samplingRateOut: Double) {
        self.samplingRateIn = samplingRateIn
        self.samplingRateOut = samplingRateOut
        let st = syldet_resampler_create(samplingRateIn, samplingRateOut, 1, 0, &handle)
        if st != 0 {
            fatalError("\(String(cString: syldet_strerror(st))): \(String(cString: syldet_last_error()))")
        }
    }

    deinit {
        syldet_resampler_destroy(handle)
    }

    func resampleVector(_ data: UnsafePointer<Float>, ofLength numSamplesIn: Int) -> [Float] {
        let numSamplesOut = Int(syldet_resampler_count(handle, Int64(numSamplesIn)))
        var ret = [Float](repeating: 0.0, count: numSamplesOut)
        var produced: Int64 = 0
        let st = syldet_resample(handle, data, Int64(numSamplesIn), Int64(numSamplesIn), &ret, Int64(max(numSamplesOut, 1)), &produced)
        if st != 0 {
            fatalError("\(String(cString: syldet_strerror(st))): \(String(cString: syldet_last_error()))")
        }
        return ret
    }

    func resampleArray(_ arr: [Float]) -> [Float] {
        guard !arr.isEmpty else { return [] }
        return arr.withUnsafeBufferPointer { resampleVector($0.baseAddress!, ofLength: $0.count) }
    }
}

/// The band-limited converter (the Kaiser-windowed sinc of syldet_convert_rate_sinc_device) as a stream: the outputs of the
/// buffers and of `flush()` together are the whole recording's, bit for bit, however the device cuts it into buffers.  Outputs
/// trail inputs by zeroCrossings / (min(1, out / in) * rolloff) input samples; for live use choose zeroCrossings 8.
class ResamplerSinc: Resampler {
    let samplingRateIn: Double
    let samplingRateOut: Double
    private var handle: OpaquePointer?

    init(fromRate samplingRateIn: Double, toRate samplingRateOut: Double, zeroCrossings: Int32? = nil, beta: Double? = nil, rolloff: Double? = nil) {
        self.samplingRateIn = samplingRateIn
        self.samplingRateOut = samplingRateOut
        var z: Int32 = 0, b = 0.0, r = 0.0
        syldet_sinc_defaults(&z, &b, &r)
        ResamplerSinc.check(syldet_sinc_resampler_create(samplingRateIn, samplingRateOut, 1, 0, zeroCrossings ?? z, beta ?? b, rolloff ?? r, &handle))
    }

    deinit {
        syldet_sinc_resampler_destroy(handle)
    }

    private static func check(_ st: Int32) {
        if st != 0 {
            fatalError("\(String(cString: syldet_strerror(st))): \(String(cString: syldet_last_error()))")
        }
    }

    func resampleVector(_ data: UnsafePointer<Float>, ofLength numSamplesIn: Int) -> [Float] {
        let numSamplesOut = Int(syldet_sinc_resampler_count(handle, Int64(numSamplesIn)))
        var ret = [Float](repeating: 0.0, count: numSamplesOut)
        var produced: Int64 = 0
        ResamplerSinc.check(syldet_sinc_resample(handle, data, Int64(numSamplesIn), Int64(numSamplesIn), &ret, Int64(max(numSamplesOut, 1)), &produced))
        return ret
    }

    func resampleArray(_ arr: [Float]) -> [Float] {
        guard !arr.isEmpty else { return [] }
        return arr.withUnsafeBufferPointer { resampleVector($0.baseAddress!, ofLength: $0.count) }
    }

    /// The recording's last outputs; afterwards only `reset()` reopens the stream.
    func flush() -> [Float] {
        let numSamplesOut = Int(syldet_sinc_resampler_flush_count(handle))
        var ret = [Float](repeating: 0.0, count: numSamplesOut)
        var produced: Int64 = 0
        ResamplerSinc.check(syldet_sinc_resampler_flush(handle, &ret, Int64(max(numSamplesOut, 1)), &produced))
        return ret
    }

    func reset() {
        ResamplerSinc.check(syldet_sinc_resampler_reset(handle))
    }
}
