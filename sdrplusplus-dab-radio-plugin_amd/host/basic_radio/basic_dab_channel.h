// basic_radio/basic_dab_channel.h -- a DAB (MPEG-1/2 layer II) audio sub-channel after the channel decoder.
// A logical frame of such a sub-channel IS one MP2 audio frame (24 ms at 48 kHz; two logical frames at 24 kHz),
// so there is nothing to reassemble: the channel checks the MPEG header of every frame, keeps what the GUI shows
// through GetAudioParams() (/root/reference/src/render_radio_block.cpp:439-460) and hands the frames to whoever
// decodes MP2 (not part of the hot path; OnAudioData() never fires).  These services normally sit on UEP
// sub-channels.
// GetDynamicLabel() and the slideshow manager (/root/reference/src/render_radio_block.cpp:470-486) are read from the
// frames' PAD without an audio decoder, by the code the GPU batch call dabgpu_mp2_follow_dev runs
// (include/dabgpu_mp2_frame.h: header valid for the sub-channel's bit rate, ISO CRC over allocation and SCFSI, the PAD
// lifted into a row) and the two walks behind it (basic_pad_reader.h).  Frame by frame there is no vote: a logical frame
// with a valid 24 kHz header waits for its second half; if the next one has such a header too, the one that waited was
// an orphan (a lost access unit) and the new one waits.  Frames without the ISO CRC (protection bit 1) deliver no PAD.
// GetAudioLevel() answers whether audio is on the channel and how loud: while audio decoding is enabled every good frame
// goes through the serial decoder of include/dabgpu_mp2_audio.h (the code the GPU batch call dabgpu_mp2_subbands_dev runs a
// lane per cell) to its sub-band samples' power and peak; the synthesis filter to PCM is not part of it.
#pragma once
#include <cstdint>
#include <memory>
#include <optional>
#include <vector>
#include "basic_radio/basic_audio_channel.h"
#include "basic_radio/basic_pad_reader.h"
#include "dabgpu_mp2_audio.h"
#include "dabgpu_mp2_frame.h"

// what the GUI prints about a layer-II stream (/root/reference/src/render_radio_block.cpp:444-467): the names of the
// reference's MP2 decoder front end; only the frame header is parsed here
struct MP2_Audio_Decoder {
    enum class MPEG_Version : uint8_t { MPEG_1_0, MPEG_2_0, MPEG_2_5 };
    enum class MPEG_Layer : uint8_t { LAYER_I, LAYER_II, LAYER_III };
    struct AudioParams {
        MPEG_Version mpeg_version = MPEG_Version::MPEG_1_0;
        MPEG_Layer mpeg_layer = MPEG_Layer::LAYER_II;
        uint32_t sample_rate = 0;
        uint32_t bitrate_kbps = 0;
        bool is_stereo = false;
    };
};

class Basic_DAB_Channel : public Basic_Audio_Channel {
public:
    Basic_DAB_Channel(const Subchannel &subchannel, int bitrate_kbps)
        : m_subchannel(subchannel), m_lf_bytes(size_t(bitrate_kbps) * 3) {}
    AudioServiceType GetType() const override { return AudioServiceType::DAB; }
    void Process(tcb::span<const uint8_t> lf) {
        if (lf.size() != m_lf_bytes || lf.size() < 4) return;
        m_total_frames++;
        // ISO 11172-3 header: 12 sync bits, ID (1 = MPEG-1 48 kHz, 0 = MPEG-2 LSF 24 kHz in DAB), layer II = 10b,
        // protection, bit-rate index, sampling frequency (01b = 48/24 kHz), padding, private, mode (11b = mono)
        static const uint16_t BITRATES_V1[16] = {0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 0};
        static const uint16_t BITRATES_V2[16] = {0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 0};
        const bool sync = lf[0] == 0xFF && (lf[1] & 0xF0) == 0xF0;
        const bool layer2 = ((lf[1] >> 1) & 3) == 2;
        const bool fs_ok = ((lf[2] >> 2) & 3) == 1;
        m_read_data = m_controls.GetIsDecodeData();
        m_read_audio = m_controls.GetIsDecodeAudio();
        if (m_read_data || m_read_audio) ReadPad(lf);
        if (!(sync && layer2 && fs_ok)) {
            m_total_header_errors++;
            m_is_error = true;
            return;
        }
        m_is_error = false;
        const bool v1 = (lf[1] & 0x08) != 0;
        MP2_Audio_Decoder::AudioParams p;
        p.mpeg_version = v1 ? MP2_Audio_Decoder::MPEG_Version::MPEG_1_0 : MP2_Audio_Decoder::MPEG_Version::MPEG_2_0;
        p.mpeg_layer = MP2_Audio_Decoder::MPEG_Layer::LAYER_II;
        p.sample_rate = v1 ? 48000u : 24000u;
        p.bitrate_kbps = (v1 ? BITRATES_V1 : BITRATES_V2)[lf[2] >> 4];
        p.is_stereo = ((lf[3] >> 6) & 3) != 3;
        m_params = p;
        if (m_controls.GetIsDecodeAudio()) m_obs_frame.Notify(lf);
    }
    const std::optional<MP2_Audio_Decoder::AudioParams> &GetAudioParams() const { return m_params; }
    bool GetIsError() const { return m_is_error; }
    // one MPEG layer II frame (as transmitted, header first)
    Observable<tcb::span<const uint8_t>> &OnMP2Frame() { return m_obs_frame; }
    int GetTotalFrames() const { return m_total_frames; }
    int GetTotalHeaderErrors() const { return m_total_header_errors; }
    const Subchannel &GetSubchannel() const { return m_subchannel; }
    // what the PAD path counted: audio frames with a good ISO CRC | with a valid header and a bad one | without the CRC
    int GetTotalCheckedFrames() const { return m_total_checked; }
    int GetTotalCrcErrors() const { return m_total_crc_errors; }
    int GetTotalFramesWithoutCrc() const { return m_total_no_crc; }
    int GetDynamicLabelCharset() const { return m_pad ? m_pad->GetLabel().charset : 0; }
    // the level record of the last good frame seen while audio decoding was enabled (sub-band domain, include/dabgpu_mp2_audio.h)
    const std::optional<dabgpu_mp2::Level> &GetAudioLevel() const { return m_level; }

private:
    // one logical frame through the shared header: a 48 kHz frame, or a half of a 24 kHz one
    void ReadPad(tcb::span<const uint8_t> lf) {
        namespace mp2 = dabgpu_mp2;
        const int lf_bytes = int(m_lf_bytes), B = lf_bytes / 3;
        if (!mp2::bitrate_ok(B)) return;
        const bool starts_24k = mp2::header_id(mp2::header_word(lf[0], lf[1], lf[2], lf[3]), B) == 0;
        if (!m_half.empty() && !starts_24k) {
            const mp2::TwoPart pair = {m_half.data(), lf.data(), lf_bytes};
            AudioFrame(pair, 2 * lf_bytes, B, 0);
            m_half.clear();
            return;
        }
        if (!m_half.empty() && m_read_data) Lost();                        // an orphan first half
        if (starts_24k) {
            m_half.assign(lf.begin(), lf.end());
            return;
        }
        const mp2::TwoPart whole = {lf.data(), lf.data(), lf_bytes};
        AudioFrame(whole, lf_bytes, B, 1);
    }
    void AudioFrame(const dabgpu_mp2::TwoPart &f, int L, int B, int id) {
        namespace mp2 = dabgpu_mp2;
        int c = 0;
        const int kind = mp2::parse_frame(f, L, B, id, &c);
        if (m_read_audio && kind == mp2::FRAME_GOOD) m_level = mp2::decode_frame(f, L, B, id, static_cast<float *>(nullptr));
        if (!m_read_data) return;
        m_total_crc_errors += kind == mp2::FRAME_CRC_FAILED;
        m_total_no_crc += kind == mp2::FRAME_NO_CRC;
        if (kind != mp2::FRAME_GOOD) return Lost();
        m_total_checked++;
        const int x = mp2::xpad_bytes(L, c);
        uint8_t row[mp2::ROW_BYTES];
        for (int j = 0; j < mp2::ROW_BYTES; j++) row[j] = mp2::row_byte(f, L, c, x, j);
        if (!m_pad) m_pad = std::make_unique<Basic_Pad_Reader>();
        m_pad->Walk(row, x + 4, m_slideshows);                             // (the access unit without the two bytes that stand for its CRC)
        const dabgpu_pad::Label &label = m_pad->GetLabel();
        m_dynamic_label.assign(reinterpret_cast<const char *>(label.text), size_t(label.length));
    }
    void Lost() {
        if (m_pad) m_pad->Walk(nullptr, -1, m_slideshows);                 // (before the first good frame there is nothing to drop)
    }
    const Subchannel m_subchannel;
    const size_t m_lf_bytes;
    std::optional<MP2_Audio_Decoder::AudioParams> m_params;
    bool m_is_error = false;
    int m_total_frames = 0, m_total_header_errors = 0;
    Observable<tcb::span<const uint8_t>> m_obs_frame;
    std::vector<uint8_t> m_half;           // the first logical frame of a 24 kHz frame, waiting for the second
    std::unique_ptr<Basic_Pad_Reader> m_pad;
    int m_total_checked = 0, m_total_crc_errors = 0, m_total_no_crc = 0;
    bool m_read_data = false, m_read_audio = false;                       // the controls, as Process found them
    std::optional<dabgpu_mp2::Level> m_level;
};
