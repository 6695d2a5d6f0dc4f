// dab/database/dab_database.h -- what BasicRadio::GetDatabase() returns
// (/root/reference/src/render_radio_block.cpp:158, 239, 491, 781).
#pragma once
#include <vector>
#include "dab/database/dab_database_entities.h"

// A service component in packet mode (FIG 0/2 TMId = 3, described by FIG 0/3); kept in a list of its own: the audio
// components, their statistics and the text dump are what they were without it.
struct PacketComponent {
    uint16_t scid = 0;                     // the 12-bit service component identifier both FIGs carry
    bool has_service = false;              // FIG 0/2 has named it
    uint32_t service_id = 0;
    bool service_id_32 = false;
    bool is_primary = false;
    bool is_described = false;             // FIG 0/3 has described it
    subchannel_id_t subchannel_id = 0;
    uint16_t packet_address = 0;
    uint8_t dscty = 0;                     // data service component type; 60 = MOT
    bool dg_flag = false;                  // false: data groups are used
};

// A stream-mode data component (FIG 0/2 TMId = 1); kept in a list of its own, as the packet-mode components are: the audio
// components, their statistics and the text dump are what they were without it.
struct StreamDataComponent {
    uint32_t service_id = 0;
    bool service_id_32 = false;
    subchannel_id_t subchannel_id = 0;
    uint8_t dscty = 0;                     // data service component type; 24 = MPEG-2 transport stream (T-DMB)
    bool is_primary = false;
    bool ca_flag = false;
};

// FIG 0/13: a user application of a service component (SId, SCIdS); kept as sent, not interpreted.  Registered types it is
// useful to know (TS 101 756): 0x002 slideshow, 0x004 TPEG, 0x007 SPI, 0x00D filecasting, 0x44A Journaline.
struct UserApplication {
    uint32_t service_id = 0;
    bool service_id_32 = false;
    uint8_t scids = 0;
    uint16_t type = 0;                     // 11 bits
    std::vector<uint8_t> data;             // user application data, 0 .. 23 bytes
};
// FIG 0/8: which component (SId, SCIdS) is: a sub-channel (short form) or a packet-mode component's SCId (long form)
struct ComponentGlobal {
    uint32_t service_id = 0;
    uint8_t scids = 0;
    bool is_packet = false;
    uint16_t id = 0;                       // SubChId (6 bits) or SCId (12 bits)
};

struct DAB_Database {
    Ensemble ensemble;
    std::vector<Service> services;
    std::vector<ServiceComponent> service_components;
    std::vector<Subchannel> subchannels;
    std::vector<LinkService> link_services;        // render_radio_block.cpp:601
    std::vector<FM_Service> fm_services;           // :628
    std::vector<DRM_Service> drm_services;         // :667
    std::vector<OtherEnsemble> other_ensembles;
    std::vector<PacketComponent> packet_components;        // render_radio_block.cpp:533 asks for their channels
    std::vector<StreamDataComponent> stream_components;    // FIG 0/2 TMId 1, each SubChId once (its first component)
    uint8_t fec_scheme[64] = {};                           // FIG 0/14, by SubChId; 0 = none announced
    std::vector<UserApplication> user_applications;        // FIG 0/13, each (SId, SCIdS, type) once
    std::vector<ComponentGlobal> component_globals;        // FIG 0/8, each (SId, SCIdS) once

    // the user applications of a packet-mode component: FIG 0/13 joined through FIG 0/8's (SId, SCIdS) to its SCId
    std::vector<const UserApplication *> UserApplicationsOf(const PacketComponent &pc) const {
        std::vector<const UserApplication *> out;
        for (const auto &g : component_globals) {
            if (!g.is_packet || g.id != pc.scid) continue;
            for (const auto &ua : user_applications)
                if (ua.service_id == g.service_id && ua.scids == g.scids) out.push_back(&ua);
        }
        return out;
    }
    // ... and of a stream-mode component, through its SubChId
    std::vector<const UserApplication *> UserApplicationsOfSubchannel(subchannel_id_t id) const {
        std::vector<const UserApplication *> out;
        for (const auto &g : component_globals) {
            if (g.is_packet || g.id != id) continue;
            for (const auto &ua : user_applications)
                if (ua.service_id == g.service_id && ua.scids == g.scids) out.push_back(&ua);
        }
        return out;
    }
};

struct DAB_Database_Statistics {           // GetDatabaseStatistics(), render_radio_block.cpp:755
    size_t nb_total = 0;                   // entity fields written
    size_t nb_pending = 0;                 // entities still missing something the FIC has yet to say (label, sub-channel)
    size_t nb_completed = 0;               // entities that are complete
    size_t nb_conflicts = 0;               // a field that was already set arrived with a different value
    size_t nb_updates = 0;                 // writes that changed something
};
