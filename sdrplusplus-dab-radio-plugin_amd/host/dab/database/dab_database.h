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
    uint8_t fec_scheme[64] = {};                           // FIG 0/14, by SubChId; 0 = none announced
};

struct DAB_Database_Statistics {           // GetDatabaseStatistics(), render_radio_block.cpp:755
    size_t nb_total = 0;                   // entity fields written
    size_t nb_pending = 0;                 // entities still missing something the FIC has yet to say (label, sub-channel)
    size_t nb_completed = 0;               // entities that are complete
    size_t nb_conflicts = 0;               // a field that was already set arrived with a different value
    size_t nb_updates = 0;                 // writes that changed something
};
