//  SyllableDetector.swift (libsyldet shim)
//
//  Drop-in for Common/SyllableDetector.swift of gardner-lab/syllable-detector-swift: same class
//  name and the members its callers use (Processor.swift:58,120,124,136-141; TrackDetector.swift:33,62,
//  65-77; ViewControllerSimulator.swift:172,292,311,322), with the arithmetic done by libsyldet on an
//  MI355X through the C ABI in include/syldet.h.  The header is imported the way the reference imports
//  TPCircularBuffer.h: one more line in Common/Common-Bridging-Header.h (#include "syldet.h").
//
//  Not compiled in this repository (no Swift toolchain in the build image); INTEGRATION.md shows where
//  it goes.  Every member the reference's callers touch is here: init(config:), config, audioSettings,
//  processSampleBuffer, captureOutput, appendAudioData, processNewValue, lastOutputs, lastDetected, seenSyllable.  One SyllableDetector here owns a one-channel bank; Processor-style callers that hold many
//  channels should create one bank for all of them (see SyllableDetectorBank below) so that a batch of
//  channels is a single kernel launch.

import Foundation
import AVFoundation

final class SyllableDetectorBank {
    let handle: OpaquePointer
    let config: SyllableDetectorConfig
    let geometry: syldet_geometry_t

    init(config: SyllableDetectorConfig, channels: Int, device: Int32 = 0) {
        self.config = config
        var h: OpaquePointer? = nil
        let st = config.withCStruct { syldet_create($0, Int32(channels), device, Int32(SYLDET_ENGINE_AUTO.rawValue), &h) }
        guard st == 0, let hh = h else {
            // the reference calls fatalError for the same conditions (SyllableDetector.swift:47,54,59)
            fatalError(String(cString: syldet_strerror(st)) + ": " + String(cString: syldet_last_error()))
        }
        handle = hh
        var g = syldet_geometry_t()
        syldet_get_geometry(hh, &g)
        geometry = g
    }

    deinit { syldet_destroy(handle) }

    /// Live use: evaluates what every channel has pending in one device round trip; the detectors'
    /// `processNewValue()` then hand the results out (Processor.swift:128-141 calls this first).
    @discardableResult func processAll() -> Int {
        var queued: Int64 = 0
        syldet_process_all(handle, &queued)
        return Int(queued)
    }

    /// simulateNetwork (ViewControllerSimulator.swift:251-344) for every channel: the outputs, the flags and the 16-bit output
    /// track [channels][n] (output 0 over its threshold, held between evaluations) of a whole recording.
    func simulate(samples: UnsafePointer<Float>, samplesPerChannel n: Int) -> (trace: [Int16], outputs: [Float], flags: [UInt8]) {
        let c = Int(syldet_channels(handle)), e = max(0, Int(syldet_count_evals(handle, Int64(n))))
        var outputs = [Float](repeating: 0, count: max(1, c * e * Int(geometry.outputs)))
        var flags = [UInt8](repeating: 0, count: max(1, c * e)), trace = [Int16](repeating: 0, count: max(1, c * n))
        var st = syldet_run(handle, samples, Int64(n), Int64(n), &outputs, &flags)
        if st == 0 { st = syldet_trace_s16(handle, outputs, Int64(e), 0, &trace, Int64(n), Int64(n)) }
        if st != 0 { fatalError(String(cString: syldet_strerror(st)) + ": " + String(cString: syldet_last_error())) }
        return (trace, outputs, flags)
    }

    /// The rig's TTL output for a whole recording (Processor.swift:128-148, AudioInterface.swift:13-40, :442-445): the outputs, the
    /// flags, the 16-bit trigger track [channels][n] (32767 for `width` samples behind every callback buffer that saw a syllable) and
    /// every channel's rising edges.
    func rehearse(samples: UnsafePointer<Float>, samplesPerChannel n: Int, width: Int, bufferLength: Int32 = 32, latency: Int = 0)
        -> (track: [Int16], onsets: [[Int64]], outputs: [Float], flags: [UInt8]) {
        let c = Int(syldet_channels(handle)), e = max(0, Int(syldet_count_evals(handle, Int64(n))))
        var outputs = [Float](repeating: 0, count: max(1, c * e * Int(geometry.outputs)))
        var flags = [UInt8](repeating: 0, count: max(1, c * e)), track = [Int16](repeating: 0, count: max(1, c * n))
        let cap = max(1, min(e, n / Int(bufferLength) + 1))
        var idx = [Int64](repeating: 0, count: c * cap), counts = [Int64](repeating: 0, count: c)
        var st = syldet_run(handle, samples, Int64(n), Int64(n), &outputs, &flags)
        if st == 0 { st = syldet_trigger_s16(handle, flags, Int64(e), bufferLength, Int64(width), Int64(latency), &track, Int64(n), Int64(n)) }
        if st == 0 { st = syldet_trigger_onsets(handle, flags, Int64(e), bufferLength, Int64(width), Int64(latency), Int64(n), &idx, Int64(cap), &counts) }
        if st != 0 { fatalError(String(cString: syldet_strerror(st)) + ": " + String(cString: syldet_last_error())) }
        return (track, (0..<c).map { ch in Array(idx[(ch * cap)..<(ch * cap + min(cap, Int(counts[ch])))]) }, outputs, flags)
    }

    private func checkTrigger(_ st: Int32) {
        if st != 0 { fatalError(String(cString: syldet_strerror(st)) + ": " + String(cString: syldet_last_error())) }
    }

    /// Int(seconds * rate), createHighOutput's width (AudioInterface.swift:444); -1 below one sample
    static func triggerWidth(seconds: Double, rate: Double) -> Int { return Int(syldet_trigger_width(seconds, rate)) }

    /// The trigger track [channels][n] of flags [channels][nEvals] (host buffers, blocking): 1.0 / 0.0, or 32767 / 0
    func triggerTrack(flags: UnsafePointer<UInt8>, evaluations e: Int, samplesPerChannel n: Int, width: Int, bufferLength: Int32 = 32, latency: Int = 0) -> [Float] {
        var t = [Float](repeating: 0, count: max(1, Int(syldet_channels(handle)) * n))
        checkTrigger(syldet_trigger(handle, flags, Int64(e), bufferLength, Int64(width), Int64(latency), &t, Int64(n), Int64(n)))
        return t
    }
    func triggerTrackPCM16(flags: UnsafePointer<UInt8>, evaluations e: Int, samplesPerChannel n: Int, width: Int, bufferLength: Int32 = 32, latency: Int = 0) -> [Int16] {
        var t = [Int16](repeating: 0, count: max(1, Int(syldet_channels(handle)) * n))
        checkTrigger(syldet_trigger_s16(handle, flags, Int64(e), bufferLength, Int64(width), Int64(latency), &t, Int64(n), Int64(n)))
        return t
    }
    /// the rising edges of one channel's track, as sample numbers
    func triggerOnsets(flags: UnsafePointer<UInt8>, evaluations e: Int, samplesPerChannel n: Int, width: Int, channel: Int, bufferLength: Int32 = 32, latency: Int = 0) -> [Int64] {
        let c = Int(syldet_channels(handle)), cap = max(1, min(e, n / Int(bufferLength) + 1))
        var idx = [Int64](repeating: 0, count: c * cap), counts = [Int64](repeating: 0, count: c)
        checkTrigger(syldet_trigger_onsets(handle, flags, Int64(e), bufferLength, Int64(width), Int64(latency), Int64(n), &idx, Int64(cap), &counts))
        return Array(idx[(channel * cap)..<(channel * cap + min(cap, Int(counts[channel])))])
    }
    /// device buffers, asynchronous on `hipStream`: fp32 rows, 16-bit rows, 16-bit frames [n][channels], 16-bit frames [n][2 channels]
    /// with the recording's int16 rows beside the triggers, and the onsets
    func triggerDevice(flags: UnsafePointer<UInt8>, evaluations e: Int64, bufferLength: Int32, width: Int64, latency: Int64, track: UnsafeMutablePointer<Float>, samplesPerChannel n: Int64, stride: Int64, hipStream: UnsafeMutableRawPointer?) {
        checkTrigger(syldet_trigger_device(handle, flags, e, bufferLength, width, latency, track, n, stride, hipStream))
    }
    func triggerDevicePCM16(flags: UnsafePointer<UInt8>, evaluations e: Int64, bufferLength: Int32, width: Int64, latency: Int64, track: UnsafeMutablePointer<Int16>, samplesPerChannel n: Int64, stride: Int64, hipStream: UnsafeMutableRawPointer?) {
        checkTrigger(syldet_trigger_device_s16(handle, flags, e, bufferLength, width, latency, track, n, stride, hipStream))
    }
    func triggerInterleavedDevicePCM16(flags: UnsafePointer<UInt8>, evaluations e: Int64, bufferLength: Int32, width: Int64, latency: Int64, frames: UnsafeMutablePointer<Int16>, samplesPerChannel n: Int64, hipStream: UnsafeMutableRawPointer?) {
        checkTrigger(syldet_trigger_interleaved_device_s16(handle, flags, e, bufferLength, width, latency, frames, n, hipStream))
    }
    func triggerMuxDevicePCM16(flags: UnsafePointer<UInt8>, evaluations e: Int64, bufferLength: Int32, width: Int64, latency: Int64, samples: UnsafePointer<Int16>, channelStride: Int64, frames: UnsafeMutablePointer<Int16>, samplesPerChannel n: Int64, hipStream: UnsafeMutableRawPointer?) {
        checkTrigger(syldet_trigger_mux_device_s16(handle, flags, e, bufferLength, width, latency, samples, channelStride, frames, n, hipStream))
    }
    func triggerOnsetsDevice(flags: UnsafePointer<UInt8>, evaluations e: Int64, bufferLength: Int32, width: Int64, latency: Int64, samplesPerChannel n: Int64, indices: UnsafeMutablePointer<Int64>?, capacity: Int64, counts: UnsafeMutablePointer<Int64>, hipStream: UnsafeMutableRawPointer?) {
        checkTrigger(syldet_trigger_onsets_device(handle, flags, e, bufferLength, width, latency, n, indices, capacity, counts, hipStream))
    }

    /// createHighOutput (AudioInterface.swift:442-445) and renderOutput (:13-40) of one channel
    func armTrigger(channel: Int32, width: Int) { checkTrigger(syldet_trigger_arm(handle, channel, Int64(width))) }
    func renderTrigger(channel: Int32, into out: UnsafeMutablePointer<Float>, frames: Int32) { checkTrigger(syldet_trigger_render(handle, channel, out, frames)) }
}

/// One bank over several MI355X of this host, one process: the reference is one process that owns every channel
/// (Processor.swift:57-59 builds a detector per channel, one serial queue drains them all :82,:128-141; main.swift:86-89,
/// :126-130 likewise per track).  The library places a sub-bank and a stream on every listed device, splits the channels into
/// contiguous blocks (time-axis ranges with a halo when there are fewer channels than devices), queues every shard's work
/// before waiting on any, and gathers the detection flags with ONE ncclAllGather of their bits per batch (device form).
///
///     let bank = SyllableDetectorShardedBank(config: config, channels: 4096, devices: [0, 1, 2, 3, 4, 5, 6, 7])
///     let (outputs, flags) = bank.run(samples: recording, samplesPerChannel: n)     // [C][n] in, [C][E][outputs] and [C][E] out
final class SyllableDetectorShardedBank {
    let handle: OpaquePointer
    let config: SyllableDetectorConfig
    let channels: Int
    let outputsPerEvaluation: Int

    init(config: SyllableDetectorConfig, channels: Int, devices: [Int32]) {
        self.config = config
        self.channels = channels
        var h: OpaquePointer? = nil
        let st = config.withCStruct { c in
            devices.withUnsafeBufferPointer { d in
                syldet_create_sharded(c, Int32(channels), d.baseAddress, Int32(d.count), Int32(SYLDET_ENGINE_AUTO.rawValue),
                                      Int32(SYLDET_EXCHANGE_RCCL.rawValue), &h)
            }
        }
        guard st == 0, let hh = h else {
            fatalError(String(cString: syldet_strerror(st)) + ": " + String(cString: syldet_last_error()))
        }
        handle = hh
        var g = syldet_geometry_t()
        syldet_get_geometry(syldet_sharded_bank(hh, 0), &g)
        outputsPerEvaluation = Int(g.outputs)
    }

    deinit { syldet_sharded_destroy(handle) }

    /// Brings the flag exchange up now (RCCL communicators over the bank's devices) instead of inside the first batch that
    /// gathers; false where that fails -- the application may then make the bank again for the copy exchange.
    func connect() -> Bool { return syldet_sharded_connect(handle) == 0 }

    func countEvaluations(samplesPerChannel n: Int) -> Int {
        return max(0, Int(syldet_count_evals(syldet_sharded_bank(handle, 0), Int64(n))))
    }

    /// The whole bank in one call on host buffers ([channels][samplesPerChannel], channel-major): every device's copies and
    /// kernels are in flight together; results land in the caller's rows (no collective in this form).
    func run(samples: UnsafePointer<Float>, samplesPerChannel n: Int) -> (outputs: [Float], flags: [UInt8]) {
        let e = countEvaluations(samplesPerChannel: n)
        var outputs = [Float](repeating: 0, count: channels * e * outputsPerEvaluation)
        var flags = [UInt8](repeating: 0, count: channels * e)
        let st = syldet_sharded_run(handle, samples, Int64(n), Int64(n), &outputs, &flags)
        if st != 0 { fatalError(String(cString: syldet_strerror(st)) + ": " + String(cString: syldet_last_error())) }
        return (outputs, flags)
    }
}

class SyllableDetector: NSObject, AVCaptureAudioDataOutputSampleBufferDelegate {
    let config: SyllableDetectorConfig
    private let bank: SyllableDetectorBank
    private let channel: Int32

    /// What a reader must deliver to this detector (the role of Common/SyllableDetector.swift:19-23; read by
    /// TrackDetector.swift:35 and ViewControllerSimulator.swift:176): packed 32-bit float PCM, one plane per channel,
    /// already at the network's sampling rate -- libsyldet's rings take exactly that layout.
    var audioSettings: [String: AnyObject] {
        var wanted = [String: AnyObject]()
        wanted[AVFormatIDKey] = NSNumber(value: kAudioFormatLinearPCM)
        wanted[AVSampleRateKey] = NSNumber(value: config.samplingRate)
        wanted[AVLinearPCMBitDepthKey] = NSNumber(value: MemoryLayout<Float>.size * 8)
        wanted[AVLinearPCMIsFloatKey] = NSNumber(value: true)
        wanted[AVLinearPCMIsNonInterleaved] = NSNumber(value: true)
        return wanted
    }

    var lastOutputs: [Float] {
        var out = [Float](repeating: 0.0, count: Int(bank.geometry.outputs))
        syldet_last_outputs(bank.handle, channel, &out)
        return out
    }
    var lastDetected: Bool { return syldet_last_detected(bank.handle, channel) == 1 }

    init(config: SyllableDetectorConfig) {
        self.config = config
        bank = SyllableDetectorBank(config: config, channels: 1)
        channel = 0
        super.init()
    }

    init(bank: SyllableDetectorBank, channel: Int) {
        config = bank.config
        self.bank = bank
        self.channel = Int32(channel)
        super.init()
    }

    func appendAudioData(_ data: UnsafeMutablePointer<Float>, withSamples numSamples: Int) {
        if syldet_append(bank.handle, channel, data, Int64(numSamples)) != 0 {
            fatalError("Insufficient space on buffer.")      // CircularShortTimeFourierTransform.swift:199
        }
    }

    /// The role of Common/SyllableDetector.swift:81-119 (callers: TrackDetector.swift:62, ViewControllerSimulator.swift:292):
    /// refuse anything but planar 32-bit float PCM the way the reference does (fatalError), then hand the buffer's samples to
    /// this channel's ring.  Like the reference (:104-118) it reads the FIRST plane of the buffer: a non-interleaved buffer with
    /// several channels (the format check lets those through, as the reference's does, and the reader settings do not pin the
    /// channel count) has one plane per channel, plane 0 first.  The audio buffer list is sized for every plane the buffer
    /// holds (a list for one buffer would fail with kCMSampleBufferError_ArrayTooSmall on a stereo file), the block buffer it
    /// retains is kept alive across the append (with Assure16ByteAlignment the data may be a copy that only the block owns),
    /// and a buffer whose samples cannot be reached falls back to the reference's own route, the block's data pointer.
    func processSampleBuffer(_ sampleBuffer: CMSampleBuffer) {
        let frames = CMSampleBufferGetNumSamples(sampleBuffer)
        if frames <= 0 { return }
        guard let desc = CMSampleBufferGetFormatDescription(sampleBuffer),
              let asbd = CMAudioFormatDescriptionGetStreamBasicDescription(desc)?.pointee else { return }
        let planar = asbd.mChannelsPerFrame <= 1 || (asbd.mFormatFlags & kAudioFormatFlagIsNonInterleaved) != 0
        let float32 = asbd.mFormatID == kAudioFormatLinearPCM && (asbd.mFormatFlags & kAudioFormatFlagIsFloat) != 0 && asbd.mBitsPerChannel == 32
        if !(planar && float32) { fatalError("Invalid audio format.") }             // :100-102

        // how large a list this buffer needs (one AudioBuffer per plane)
        var needed = 0
        var st = CMSampleBufferGetAudioBufferListWithRetainedBlockBuffer(sampleBuffer, &needed, nil, 0, nil, nil, 0, nil)
        if st == noErr && needed >= MemoryLayout<AudioBufferList>.size {
            let raw = UnsafeMutableRawPointer.allocate(byteCount: needed, alignment: MemoryLayout<AudioBufferList>.alignment)
            defer { raw.deallocate() }
            let list = raw.bindMemory(to: AudioBufferList.self, capacity: 1)
            var block: CMBlockBuffer? = nil
            st = CMSampleBufferGetAudioBufferListWithRetainedBlockBuffer(sampleBuffer, nil, list, needed, nil, nil,
                                                                         kCMSampleBufferFlag_AudioBufferList_Assure16ByteAlignment, &block)
            if st == noErr, let held = block {
                let planes = UnsafeMutableAudioBufferListPointer(list)
                if let first = planes.first, let bytes = first.mData {
                    let n = min(frames, Int(first.mDataByteSize) / MemoryLayout<Float>.size)
                    withExtendedLifetime(held) {                       // the samples belong to the block: it outlives the append
                        appendAudioData(bytes.assumingMemoryBound(to: Float.self), withSamples: n)
                    }
                    return
                }
            }
        }
        // the reference's route (:104-118): the block buffer's data pointer, plane 0 at its start
        guard let audioBuffer = CMSampleBufferGetDataBuffer(sampleBuffer) else {
            NSLog("SyllableDetector: unable to get the audio buffer (status %d); %d samples dropped", Int(st), frames)
            return
        }
        var lengthAtOffset = 0, totalLength = 0
        var inSamples: UnsafeMutablePointer<Int8>? = nil
        let got = CMBlockBufferGetDataPointer(audioBuffer, 0, &lengthAtOffset, &totalLength, &inSamples)
        guard got == kCMBlockBufferNoErr, let p = inSamples, lengthAtOffset >= frames * MemoryLayout<Float>.size else {
            fatalError("Unable to read the audio buffer (status \(got)).")          // never drop audio silently: a detector that skips buffers reports wrong sample numbers
        }
        withExtendedLifetime(audioBuffer) {
            p.withMemoryRebound(to: Float.self, capacity: frames) { appendAudioData($0, withSamples: frames) }
        }
    }

    /// :121-127 (AVCaptureAudioDataOutputSampleBufferDelegate): ingest, then drain every evaluation that became available
    func captureOutput(_ captureOutput: AVCaptureOutput, didOutput sampleBuffer: CMSampleBuffer, from connection: AVCaptureConnection) {
        processSampleBuffer(sampleBuffer)
        while processNewValue() {}
    }

    func processNewValue() -> Bool { return syldet_process_new_value(bank.handle, channel) == 1 }

    func seenSyllable() -> Bool { return syldet_seen_syllable(bank.handle, channel) == 1 }
}
