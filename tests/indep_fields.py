"""A second reading of the field decode: decodeModesMessage's fields (mode_s.c:557-715), decodeExtendedSquitter and its
type decoders (mode_s.c:736-1474), decodeCommB (comm_b.c), decodeModeAMessage (mode_ac.c:168-202) and the Gillham
conversion it calls (mode_ac.c:100-163), with ais_charset.c -- written from those lines of the reference alone, in plain
Python and numpy, keeping the reference's shape: one function per message type, struct modesMessage members under their
own names, floats as floats (a C `float` is np.float32, every expression is evaluated in double and narrowed where the
reference assigns it), and comm_b.c's float comparisons as they are written there.

Two deviations in shape, none in content:
  * the Comm-B decoders take arrays (one MB field per element): a `return 0` becomes a cleared `alive` mask, a `score +=`
    an addition under a mask.  decodeCommB is called where mode_s.c:669 calls it -- after DR, before UM (mode_s.c:705), so
    the UM it tests is still zero -- but for a whole array of records at once.
  * what the reference keeps as local variables and the product delivers (the velocity components, the raw values behind
    the floats) is kept beside the members, under the locals' names.

---- from struct modesMessage to the product's msd_fields (members_of) ----
The product delivers integers where the reference stores floats.  Each raw member is the reference's local the float is
computed from:
  heading_raw       ES type 19 subtypes 3/4: getbits(me, 15, 24)  (heading = raw * 360 / 1024, mode_s.c:853)
                    ES surface position:     getbits(me, 14, 20)  (raw * 360 / 128, :922)
                    BDS 5,0 / 6,0: track_raw / heading_raw + 1024 * sign  (raw * 90 / 512 (+ 180), comm_b.c:486-489,625-628)
  heading_valid,    as in the reference, except ES type 19 subtypes 1/2 (:835-841), where the product delivers
  heading_type      velocity_valid, ew_vel, ns_vel (the locals of :827-828) and derives track and speed on the host
  movement          getbits(me, 6, 12) where gs_valid is set from it (:912), else 0
  gs                BDS 5,0 `gs` (comm_b.c:498), with commb_valid bit 2 where BDS 5,0 set gs_valid
  roll_q            roll_raw - 512 * roll_sign            (roll = raw * 45 / 256 (- 90), comm_b.c:467-470), commb_valid bit 1
  track_rate_q      track_rate_raw - 512 * track_rate_sign (raw * 8 / 256 (- 16), :513-516), commb_valid bit 4
  mach_raw          mach_raw (mach = raw * 2.048 / 512, :652), commb_valid bit 8
  nav_qnh_raw       ME type 29 v2: baro_bits (qnh = 800 + (raw - 1) * 0.8, mode_s.c:1212); BDS 4,0: baro_raw
                    (800 + raw * 0.1, comm_b.c:326) with nav_valid bit 64
  nav_heading_raw   ME type 29: getbits(me, 28, 36) (degrees, :1131), or getbits(me, 31, 39) (x 180 / 256, :1219) with
                    nav_valid bit 32
  nav_valid         modes_valid 1, heading_valid 2, mcp_altitude_valid 4, fms_altitude_valid 8, qnh_valid 16
  acc_valid         nac_p_valid 1, nic_baro_valid 2, nic_a_valid 4, nic_c_valid 8, gva_valid 16, sda_valid 32
  opstatus          valid bit 0, version 1-3, om_acas_ra 4, om_ident 5, om_atc 6, om_saf 7, cc_acas 8, cc_cdti 9,
                    cc_1090_in 10, cc_arv 11, cc_ts 12, cc_tc 13-14, cc_uat_in 15, cc_poa 16, cc_b2_low 17, cc_lw_valid 18,
                    cc_lw 19-22, hrd 23-25, tah 26-28
  imf               setIMF was called
  addr              the record's addr (what the CRC switch of mode_s.c:445-555 left, AA for DF11/17/18) with the reference's
                    later `|= MODES_NON_ICAO_ADDRESS`
  source            what the CRC switch leaves (:464,500,529,543) and the ES decoder overrides; a DF the switch refuses
                    (`default: return -2`) never becomes a message in the reference: source_known is 0 there and the
                    member is not compared
The enumerations are the reference's (readsb.h:133-195, readsb.pb-c.h:32-105).
The float members (floats_of) are the reference's own: gs.v0 / gs.v2 / gs.selected, heading, track_rate, roll, nav.qnh,
nav.heading as float, mach as double.
"""
import math

import numpy as np

from test_fields import FIELD_NAMES, FLOAT_NAMES

f32 = np.float32
M_PI = math.pi

INVALID_ALTITUDE = -9999
MODES_NON_ICAO_ADDRESS = 1 << 24
SOURCE_MODE_AC, SOURCE_MODE_S, SOURCE_MODE_S_CHECKED, SOURCE_TISB, SOURCE_ADSR, SOURCE_ADSB = 1, 3, 4, 5, 6, 7
UNIT_FEET, UNIT_METERS = 0, 1
CPR_SURFACE, CPR_AIRBORNE = 0, 1
HEADING_INVALID, HEADING_GROUND_TRACK, HEADING_TRUE, HEADING_MAGNETIC, HEADING_MAGNETIC_OR_TRUE, HEADING_TRACK_OR_HEADING = range(6)
(COMMB_UNKNOWN, COMMB_AMBIGUOUS, COMMB_EMPTY_RESPONSE, COMMB_DATALINK_CAPS, COMMB_GICB_CAPS, COMMB_AIRCRAFT_IDENT, COMMB_ACAS_RA,
 COMMB_VERTICAL_INTENT, COMMB_TRACK_TURN, COMMB_HEADING_SPEED) = range(10)
NAV_MODE_AUTOPILOT, NAV_MODE_VNAV, NAV_MODE_ALT_HOLD, NAV_MODE_APPROACH, NAV_MODE_LNAV, NAV_MODE_TCAS = 1, 2, 4, 8, 16, 32
NAV_ALT_INVALID, NAV_ALT_UNKNOWN, NAV_ALT_AIRCRAFT, NAV_ALT_MCP, NAV_ALT_FMS = range(5)
AG_INVALID, AG_GROUND, AG_AIRBORNE, AG_UNCERTAIN = range(4)
(ADDR_ADSB_ICAO, ADDR_ADSB_ICAO_NT, ADDR_ADSR_ICAO, ADDR_TISB_ICAO, ADDR_ADSB_OTHER, ADDR_ADSR_OTHER, ADDR_TISB_TRACKFILE,
 ADDR_TISB_OTHER, ADDR_MODE_A, ADDR_UNKNOWN) = range(10)
SIL_INVALID, SIL_UNKNOWN, SIL_PER_SAMPLE, SIL_PER_HOUR = range(4)

ais_charset = b"@ABCDEFGHIJKLMNOPQRSTUVWXYZ[\\]^_ !\"#$%&'()*+,-./0123456789:;<=>?"
assert len(ais_charset) == 64

# every member of struct modesMessage this reading fills (nav.x as nav_x, accuracy.x as acc_x, opstatus.x as ops_x), and
# the locals kept beside them (raw_*, ew_vel, ns_vel, imf_set, source_known); all start at zero as after the memset
MEMBERS = (
    "msgtype addr source source_known addrtype AC altitude_baro altitude_baro_unit altitude_baro_valid CA airground CC CF DR "
    "FS alert alert_valid spi spi_valid ID squawk squawk_valid KE ND RI SL UM VS metype mesub callsign_valid cpr_valid "
    "cpr_type cpr_odd cpr_lat cpr_lon altitude_geom altitude_geom_unit altitude_geom_valid category category_valid "
    "acc_nac_v_valid acc_nac_v acc_nic_b_valid acc_nic_b acc_nac_p_valid acc_nac_p acc_nic_baro_valid acc_nic_baro acc_sil "
    "acc_sil_type acc_nic_a_valid acc_nic_a acc_nic_c_valid acc_nic_c acc_gva_valid acc_gva acc_sda_valid acc_sda "
    "gs_valid gs_v0 gs_v2 gs_selected heading heading_valid heading_type tas tas_valid ias ias_valid baro_rate "
    "baro_rate_valid geom_rate geom_rate_valid geom_delta geom_delta_valid emergency emergency_valid "
    "nav_altitude_source nav_modes_valid nav_modes nav_mcp_altitude_valid nav_mcp_altitude nav_fms_altitude_valid "
    "nav_fms_altitude nav_heading_valid nav_heading nav_heading_type nav_qnh_valid nav_qnh "
    "ops_valid ops_version ops_om_acas_ra ops_om_ident ops_om_atc ops_om_saf ops_cc_acas ops_cc_cdti ops_cc_1090_in "
    "ops_cc_arv ops_cc_ts ops_cc_tc ops_cc_uat_in ops_cc_poa ops_cc_b2_low ops_cc_lw_valid ops_cc_lw ops_cc_antenna_offset "
    "ops_hrd ops_tah commb_format roll roll_valid track_rate track_rate_valid mach mach_valid "
    "imf_set velocity_set ew_vel ns_vel raw_heading raw_movement raw_gs raw_roll raw_track_rate raw_mach raw_qnh "
    "raw_qnh_commb raw_nav_heading raw_nav_heading_v2").split()
FLOAT_MEMBERS = {"gs_v0", "gs_v2", "gs_selected", "heading", "nav_heading", "nav_qnh", "roll", "track_rate", "mach"}


class MM:
    """struct modesMessage after its memset"""
    callsign = b"\0" * 8


for _m in MEMBERS:
    setattr(MM, _m, 0)


def getbits(data, firstbit, lastbit):
    """mode_s.h: bits firstbit..lastbit of data, numbered from 1 at the most significant bit of the first byte"""
    value, nbits = data
    return (value >> (nbits - lastbit)) & ((1 << (lastbit - firstbit + 1)) - 1)


def getbit(data, bit):
    return getbits(data, bit, bit)


def bits_of(raw):
    return (int.from_bytes(bytes(raw), "big"), 8 * len(raw))


# ---------------------------------------------------------------------------------------------------- mode_ac.c:100-163
def internalModeAToModeC(ModeA):
    FiveHundreds = 0
    OneHundreds = 0
    if (ModeA & 0xFFFF8889) != 0 or (ModeA & 0x000000F0) == 0:  # zero bits are zero, D1 set is illegal; C1..C4 not all zero
        return INVALID_ALTITUDE
    if ModeA & 0x0010:
        OneHundreds ^= 0x007
    if ModeA & 0x0020:
        OneHundreds ^= 0x003
    if ModeA & 0x0040:
        OneHundreds ^= 0x001
    if (OneHundreds & 5) == 5:
        OneHundreds ^= 2
    if OneHundreds > 5:
        return INVALID_ALTITUDE
    if ModeA & 0x0002:
        FiveHundreds ^= 0x0FF
    if ModeA & 0x0004:
        FiveHundreds ^= 0x07F
    if ModeA & 0x1000:
        FiveHundreds ^= 0x03F
    if ModeA & 0x2000:
        FiveHundreds ^= 0x01F
    if ModeA & 0x4000:
        FiveHundreds ^= 0x00F
    if ModeA & 0x0100:
        FiveHundreds ^= 0x007
    if ModeA & 0x0200:
        FiveHundreds ^= 0x003
    if ModeA & 0x0400:
        FiveHundreds ^= 0x001
    if FiveHundreds & 1:
        OneHundreds = 6 - OneHundreds
    return (FiveHundreds * 5) + OneHundreds - 13


def modeAToModeC(modeA):
    """mode_ac.c:81-87 over the table of :63-75: the index keeps the twelve code bits of modeA and nothing else
    (modeAToIndex / indexToModeA, track.h:247-256), so the table's entry is internalModeAToModeC of those bits"""
    return internalModeAToModeC(modeA & 0x7777)


def decodeModeAMessage(mm, ModeA):  # mode_ac.c:168-202
    mm.source = SOURCE_MODE_AC
    mm.source_known = 1
    mm.addrtype = ADDR_MODE_A
    mm.msgtype = 32
    mm.addr = (ModeA & 0x0000FF7F) | MODES_NON_ICAO_ADDRESS
    mm.squawk = ModeA & 0x7777
    mm.squawk_valid = 1
    mm.spi = 1 if (ModeA & 0x0080) else 0
    mm.spi_valid = 1
    if not mm.spi:
        modeC = modeAToModeC(ModeA)
        if modeC != INVALID_ALTITUDE:
            mm.altitude_baro = modeC * 100
            mm.altitude_baro_unit = UNIT_FEET
            mm.altitude_baro_valid = 1


# ----------------------------------------------------------------------------------------------------- mode_s.c:101-259
def decodeID13Field(ID13Field):
    hexGillham = 0
    if ID13Field & 0x1000:
        hexGillham |= 0x0010  # C1
    if ID13Field & 0x0800:
        hexGillham |= 0x1000  # A1
    if ID13Field & 0x0400:
        hexGillham |= 0x0020  # C2
    if ID13Field & 0x0200:
        hexGillham |= 0x2000  # A2
    if ID13Field & 0x0100:
        hexGillham |= 0x0040  # C4
    if ID13Field & 0x0080:
        hexGillham |= 0x4000  # A4
    if ID13Field & 0x0020:
        hexGillham |= 0x0100  # B1
    if ID13Field & 0x0010:
        hexGillham |= 0x0001  # D1 or Q
    if ID13Field & 0x0008:
        hexGillham |= 0x0200  # B2
    if ID13Field & 0x0004:
        hexGillham |= 0x0002  # D2
    if ID13Field & 0x0002:
        hexGillham |= 0x0400  # B4
    if ID13Field & 0x0001:
        hexGillham |= 0x0004  # D4
    return hexGillham


def decodeAC13Field(AC13Field):
    """-> (altitude, unit)"""
    m_bit = AC13Field & 0x0040
    q_bit = AC13Field & 0x0010
    if not m_bit:
        if q_bit:
            n = ((AC13Field & 0x1F80) >> 2) | ((AC13Field & 0x0020) >> 1) | (AC13Field & 0x000F)
            return (n * 25) - 1000, UNIT_FEET
        n = modeAToModeC(decodeID13Field(AC13Field))
        if n < -12:
            return INVALID_ALTITUDE, UNIT_FEET
        return 100 * n, UNIT_FEET
    return INVALID_ALTITUDE, UNIT_METERS


def decodeAC12Field(AC12Field):
    q_bit = AC12Field & 0x10
    if q_bit:
        n = ((AC12Field & 0x0FE0) >> 1) | (AC12Field & 0x000F)
        return (n * 25) - 1000, UNIT_FEET
    n = ((AC12Field & 0x0FC0) << 1) | (AC12Field & 0x003F)
    n = modeAToModeC(decodeID13Field(n))
    if n < -12:
        return INVALID_ALTITUDE, UNIT_FEET
    return 100 * n, UNIT_FEET


def decodeMovementFieldV2(movement):  # returns float: the double expression narrowed by `return`
    if movement >= 125:
        return f32(0)
    elif movement == 124:
        return f32(180)
    elif movement >= 109:
        return f32(100 + (movement - 109 + 0.5) * 5)
    elif movement >= 94:
        return f32(70 + (movement - 94 + 0.5) * 2)
    elif movement >= 39:
        return f32(15 + (movement - 39 + 0.5) * 1)
    elif movement >= 13:
        return f32(2 + (movement - 13 + 0.5) * 0.50)
    elif movement >= 9:
        return f32(1 + (movement - 9 + 0.5) * 0.25)
    elif movement >= 3:
        return f32(0.125 + (movement - 3 + 0.5) * 0.875 / 6)
    elif movement >= 2:
        return f32(0.125 / 2)
    return f32(0)


def decodeMovementFieldV0(movement):
    if movement >= 125:
        return f32(0)
    elif movement == 124:
        return f32(180)
    elif movement >= 109:
        return f32(100 + (movement - 109 + 0.5) * 5)
    elif movement >= 94:
        return f32(70 + (movement - 94 + 0.5) * 2)
    elif movement >= 39:
        return f32(15 + (movement - 39 + 0.5) * 1)
    elif movement >= 13:
        return f32(2 + (movement - 13 + 0.5) * 0.50)
    elif movement >= 9:
        return f32(1 + (movement - 9 + 0.5) * 0.25)
    elif movement >= 2:
        return f32(0.125 + (movement - 2 + 0.5) * 0.125)
    return f32(0)


# ---------------------------------------------------------------------------------------------------- mode_s.c:736-1474
def decodeESIdentAndCategory(mm, me):
    mm.mesub = getbits(me, 6, 8)
    mm.callsign = bytes(ais_charset[getbits(me, 9 + 6 * i, 14 + 6 * i)] for i in range(8))
    mm.callsign_valid = 1
    for c in mm.callsign:
        if not (ord("A") <= c <= ord("Z")) and not (ord("0") <= c <= ord("9")) and c != ord(" "):
            mm.callsign_valid = 0
            break
    mm.category = ((0x0E - mm.metype) << 4) | mm.mesub
    mm.category_valid = 1


def setIMF(mm):
    mm.addr |= MODES_NON_ICAO_ADDRESS
    mm.imf_set = 1
    if mm.addrtype in (ADDR_ADSB_ICAO, ADDR_ADSB_ICAO_NT):
        mm.addrtype = ADDR_ADSB_OTHER
    elif mm.addrtype == ADDR_TISB_ICAO:
        mm.addrtype = ADDR_TISB_TRACKFILE
    elif mm.addrtype == ADDR_ADSR_ICAO:
        mm.addrtype = ADDR_ADSR_OTHER


def decodeESAirborneVelocity(mm, me, check_imf):
    mm.mesub = getbits(me, 6, 8)
    if mm.mesub < 1 or mm.mesub > 4:
        return
    if check_imf and getbit(me, 9):
        setIMF(mm)
    mm.acc_nac_v_valid = 1
    mm.acc_nac_v = getbits(me, 11, 13)
    if mm.mesub in (1, 2):
        ew_raw = getbits(me, 15, 24)
        ns_raw = getbits(me, 26, 35)
        if ew_raw and ns_raw:
            ew_vel = (ew_raw - 1) * (-1 if getbit(me, 14) else 1) * (4 if mm.mesub == 2 else 1)
            ns_vel = (ns_raw - 1) * (-1 if getbit(me, 25) else 1) * (4 if mm.mesub == 2 else 1)
            # sqrtf of the double (int + int + 0.5): the argument is narrowed to float, the root is a float's
            mm.gs_v0 = mm.gs_v2 = mm.gs_selected = np.sqrt(f32((ns_vel * ns_vel) + (ew_vel * ew_vel) + 0.5))
            mm.gs_valid = 1
            mm.velocity_set, mm.ew_vel, mm.ns_vel = 1, ew_vel, ns_vel
            if mm.gs_selected > 0:
                ground_track = f32(math.atan2(ew_vel, ns_vel) * 180.0 / M_PI)
                if ground_track < 0:
                    ground_track = f32(ground_track + f32(360))
                mm.heading = ground_track
                mm.heading_type = HEADING_GROUND_TRACK
                mm.heading_valid = 1
    else:
        if getbit(me, 14):
            mm.heading_valid = 1
            mm.raw_heading = getbits(me, 15, 24)
            mm.heading = f32(getbits(me, 15, 24) * 360.0 / 1024.0)
            mm.heading_type = HEADING_MAGNETIC_OR_TRUE
        airspeed = getbits(me, 26, 35)
        if airspeed:
            speed = (airspeed - 1) * (4 if mm.mesub == 4 else 1)
            if getbit(me, 25):
                mm.tas_valid = 1
                mm.tas = speed
            else:
                mm.ias_valid = 1
                mm.ias = speed
    vert_rate = getbits(me, 38, 46)
    vert_rate_is_baro = getbit(me, 36)
    if vert_rate:
        rate = (vert_rate - 1) * (-64 if getbit(me, 37) else 64)
        if vert_rate_is_baro:
            mm.baro_rate = rate
            mm.baro_rate_valid = 1
        else:
            mm.geom_rate = rate
            mm.geom_rate_valid = 1
    raw_delta = getbits(me, 50, 56)
    if raw_delta:
        mm.geom_delta_valid = 1
        mm.geom_delta = (raw_delta - 1) * (-25 if getbit(me, 49) else 25)


def decodeESSurfacePosition(mm, me, check_imf):
    mm.airground = AG_GROUND
    mm.cpr_valid = 1
    mm.cpr_type = CPR_SURFACE
    movement = getbits(me, 6, 12)
    if movement > 0 and movement < 125:
        mm.gs_valid = 1
        mm.gs_selected = mm.gs_v0 = decodeMovementFieldV0(movement)
        mm.gs_v2 = decodeMovementFieldV2(movement)
        mm.raw_movement = movement
    if getbit(me, 13):
        mm.heading_valid = 1
        mm.raw_heading = getbits(me, 14, 20)
        mm.heading = f32(getbits(me, 14, 20) * 360.0 / 128.0)
        mm.heading_type = HEADING_TRACK_OR_HEADING
    if check_imf and getbit(me, 21):
        setIMF(mm)
    mm.cpr_odd = getbit(me, 22)
    mm.cpr_lat = getbits(me, 23, 39)
    mm.cpr_lon = getbits(me, 40, 56)


def decodeESAirbornePosition(mm, me, check_imf):
    ss = getbits(me, 6, 7)
    if ss == 0:
        mm.alert_valid = mm.spi_valid = 1
        mm.alert = mm.spi = 0
    elif ss in (1, 2):
        mm.alert_valid = 1
        mm.alert = 1
    elif ss == 3:
        mm.alert_valid = mm.spi_valid = 1
        mm.alert = 0
        mm.spi = 1
    if check_imf:
        if getbit(me, 8):
            setIMF(mm)
    else:
        mm.acc_nic_b_valid = 1
        mm.acc_nic_b = getbit(me, 8)
    AC12Field = getbits(me, 9, 20)
    if mm.metype == 0:
        pass
    else:
        mm.cpr_lat = getbits(me, 23, 39)
        mm.cpr_lon = getbits(me, 40, 56)
        if AC12Field == 0 and mm.cpr_lon == 0 and (mm.cpr_lat & 0x0fff) == 0 and mm.metype == 15:
            pass  # a known transmitter fault, counted and not marked valid
        else:
            mm.cpr_valid = 1
            mm.cpr_type = CPR_AIRBORNE
            mm.cpr_odd = getbit(me, 22)
    if AC12Field and mm.airground != AG_GROUND:
        alt, unit = decodeAC12Field(AC12Field)
        if alt != INVALID_ALTITUDE:
            if mm.metype == 20 or mm.metype == 21 or mm.metype == 22:
                mm.altitude_geom = alt
                mm.altitude_geom_unit = unit
                mm.altitude_geom_valid = 1
            else:
                mm.altitude_baro = alt
                mm.altitude_baro_unit = unit
                mm.altitude_baro_valid = 1


def decodeESTestMessage(mm, me):
    mm.mesub = getbits(me, 6, 8)
    if mm.mesub == 7:
        ID13Field = getbits(me, 9, 21)
        if ID13Field:
            mm.squawk_valid = 1
            mm.squawk = decodeID13Field(ID13Field)


def decodeESAircraftStatus(mm, me, check_imf):
    mm.mesub = getbits(me, 6, 8)
    if mm.mesub == 1:
        mm.emergency_valid = 1
        mm.emergency = getbits(me, 9, 11)
        ID13Field = getbits(me, 12, 24)
        if ID13Field:
            mm.squawk_valid = 1
            mm.squawk = decodeID13Field(ID13Field)
        if check_imf and getbit(me, 56):
            setIMF(mm)


def decodeESTargetStatus(mm, me, check_imf):
    mm.mesub = getbits(me, 6, 7)
    if check_imf and getbit(me, 51):
        setIMF(mm)
    if mm.mesub == 0 and getbit(me, 11) == 0:  # target state and status, V1
        vs = getbits(me, 8, 9)
        if vs == 1:
            mm.nav_altitude_source = NAV_ALT_MCP
        elif vs == 2:
            mm.nav_altitude_source = NAV_ALT_AIRCRAFT
        elif vs == 3:
            mm.nav_altitude_source = NAV_ALT_FMS
        vm = getbits(me, 14, 15)
        if vm == 1:  # acquiring
            mm.nav_modes_valid = 1
            if mm.nav_altitude_source == NAV_ALT_FMS:
                mm.nav_modes |= NAV_MODE_VNAV
            else:
                mm.nav_modes |= NAV_MODE_AUTOPILOT
        elif vm == 2:  # maintaining
            mm.nav_modes_valid = 1
            if mm.nav_altitude_source == NAV_ALT_FMS:
                mm.nav_modes |= NAV_MODE_VNAV
            elif mm.nav_altitude_source == NAV_ALT_AIRCRAFT:
                mm.nav_modes |= NAV_MODE_ALT_HOLD
            else:
                mm.nav_modes |= NAV_MODE_AUTOPILOT
        alt = -1000 + 100 * getbits(me, 16, 25)
        if mm.nav_altitude_source == NAV_ALT_MCP:
            mm.nav_mcp_altitude_valid = 1
            mm.nav_mcp_altitude = alt
        elif mm.nav_altitude_source == NAV_ALT_FMS:
            mm.nav_fms_altitude_valid = 1
            mm.nav_fms_altitude = alt
        h_source = getbits(me, 26, 27)
        if h_source != 0:
            mm.nav_heading_valid = 1
            mm.raw_nav_heading = getbits(me, 28, 36)
            mm.nav_heading = f32(getbits(me, 28, 36))
            if getbit(me, 37):
                mm.nav_heading_type = HEADING_GROUND_TRACK
            else:
                mm.nav_heading_type = HEADING_MAGNETIC_OR_TRUE
        hm = getbits(me, 38, 39)
        if hm in (1, 2):
            mm.nav_modes_valid = 1
            if h_source == 3:
                mm.nav_modes |= NAV_MODE_LNAV
            else:
                mm.nav_modes |= NAV_MODE_AUTOPILOT
        mm.acc_nac_p_valid = 1
        mm.acc_nac_p = getbits(me, 40, 43)
        mm.acc_nic_baro_valid = 1
        mm.acc_nic_baro = getbit(me, 44)
        mm.acc_sil = getbits(me, 45, 46)
        mm.acc_sil_type = SIL_UNKNOWN
        tcas = getbits(me, 52, 53)
        if tcas == 1:
            mm.nav_modes_valid = 1
        elif tcas in (2, 3):
            mm.nav_modes_valid = 1
            mm.nav_modes |= NAV_MODE_TCAS
        elif tcas == 0:
            mm.nav_modes |= NAV_MODE_TCAS  # "assume TCAS if we had any other modes but don't enable modes just for this"
        mm.emergency_valid = 1
        mm.emergency = getbits(me, 54, 56)
    elif mm.mesub == 1:  # V2
        is_fms = getbit(me, 9)
        alt_bits = getbits(me, 10, 20)
        if alt_bits != 0:
            if is_fms:
                mm.nav_fms_altitude_valid = 1
                mm.nav_fms_altitude = (alt_bits - 1) * 32
            else:
                mm.nav_mcp_altitude_valid = 1
                mm.nav_mcp_altitude = (alt_bits - 1) * 32
        baro_bits = getbits(me, 21, 29)
        if baro_bits != 0:
            mm.nav_qnh_valid = 1
            mm.raw_qnh = baro_bits
            mm.nav_qnh = f32(800.0 + (baro_bits - 1) * 0.8)
        if getbit(me, 30):
            mm.nav_heading_valid = 1
            mm.raw_nav_heading = getbits(me, 31, 39)
            mm.raw_nav_heading_v2 = 1
            mm.nav_heading = f32(getbits(me, 31, 39) * 180.0 / 256.0)
            mm.nav_heading_type = HEADING_MAGNETIC_OR_TRUE
        mm.acc_nac_p_valid = 1
        mm.acc_nac_p = getbits(me, 40, 43)
        mm.acc_nic_baro_valid = 1
        mm.acc_nic_baro = getbit(me, 44)
        mm.acc_sil = getbits(me, 45, 46)
        mm.acc_sil_type = SIL_UNKNOWN
        if getbit(me, 47):
            mm.nav_modes_valid = 1
            mm.nav_modes = ((NAV_MODE_AUTOPILOT if getbit(me, 48) else 0) | (NAV_MODE_VNAV if getbit(me, 49) else 0) |
                            (NAV_MODE_ALT_HOLD if getbit(me, 50) else 0) | (NAV_MODE_APPROACH if getbit(me, 52) else 0) |
                            (NAV_MODE_TCAS if getbit(me, 53) else 0) | (NAV_MODE_LNAV if getbit(me, 54) else 0))


def decodeESOperationalStatus(mm, me, check_imf):
    mm.mesub = getbits(me, 6, 8)
    if check_imf and getbit(me, 56):
        setIMF(mm)
    if mm.mesub == 0 or mm.mesub == 1:
        mm.ops_valid = 1
        mm.ops_version = getbits(me, 41, 43)
        if mm.ops_version == 0:
            if mm.mesub == 0 and getbits(me, 9, 10) == 0:
                mm.ops_cc_acas = int(not getbit(me, 12))
                mm.ops_cc_cdti = getbit(me, 13)
        elif mm.ops_version == 1:
            if getbits(me, 25, 26) == 0:
                mm.ops_om_acas_ra = getbit(me, 27)
                mm.ops_om_ident = getbit(me, 28)
                mm.ops_om_atc = getbit(me, 29)
            if mm.mesub == 0 and getbits(me, 9, 10) == 0 and getbits(me, 13, 14) == 0:
                mm.ops_cc_acas = int(not getbit(me, 11))
                mm.ops_cc_cdti = getbit(me, 12)
                mm.ops_cc_arv = getbit(me, 15)
                mm.ops_cc_ts = getbit(me, 16)
                mm.ops_cc_tc = getbits(me, 17, 18)
            elif mm.mesub == 1 and getbits(me, 9, 10) == 0 and getbits(me, 13, 14) == 0:
                mm.ops_cc_poa = getbit(me, 11)
                mm.ops_cc_cdti = getbit(me, 12)
                mm.ops_cc_b2_low = getbit(me, 15)
                mm.ops_cc_lw_valid = 1
                mm.ops_cc_lw = getbits(me, 21, 24)
            mm.acc_nic_a_valid = 1
            mm.acc_nic_a = getbit(me, 44)
            mm.acc_nac_p_valid = 1
            mm.acc_nac_p = getbits(me, 45, 48)
            mm.acc_sil_type = SIL_UNKNOWN
            mm.acc_sil = getbits(me, 51, 52)
            mm.ops_hrd = HEADING_MAGNETIC if getbit(me, 54) else HEADING_TRUE
            if mm.mesub == 0:
                mm.acc_nic_baro_valid = 1
                mm.acc_nic_baro = getbit(me, 53)
            else:
                mm.ops_tah = mm.ops_hrd if getbit(me, 53) else HEADING_GROUND_TRACK
        elif mm.ops_version == 2:
            if getbits(me, 25, 26) == 0:
                mm.ops_om_acas_ra = getbit(me, 27)
                mm.ops_om_ident = getbit(me, 28)
                mm.ops_om_atc = getbit(me, 29)
                mm.ops_om_saf = getbit(me, 30)
                mm.acc_sda_valid = 1
                mm.acc_sda = getbits(me, 31, 32)
            if mm.mesub == 0 and getbits(me, 9, 10) == 0:
                mm.ops_cc_acas = getbit(me, 11)
                mm.ops_cc_1090_in = getbit(me, 12)
                mm.ops_cc_arv = getbit(me, 15)
                mm.ops_cc_ts = getbit(me, 16)
                mm.ops_cc_tc = getbits(me, 17, 18)
                mm.ops_cc_uat_in = getbit(me, 19)
            elif mm.mesub == 1 and getbits(me, 9, 10) == 0:
                mm.ops_cc_poa = getbit(me, 11)
                mm.ops_cc_1090_in = getbit(me, 12)
                mm.ops_cc_b2_low = getbit(me, 15)
                mm.ops_cc_uat_in = getbit(me, 16)
                mm.acc_nac_v_valid = 1
                mm.acc_nac_v = getbits(me, 17, 19)
                mm.acc_nic_c_valid = 1
                mm.acc_nic_c = getbit(me, 20)
                mm.ops_cc_lw_valid = 1
                mm.ops_cc_lw = getbits(me, 21, 24)
                mm.ops_cc_antenna_offset = getbits(me, 33, 40)
            mm.acc_nic_a_valid = 1
            mm.acc_nic_a = getbit(me, 44)
            mm.acc_nac_p_valid = 1
            mm.acc_nac_p = getbits(me, 45, 48)
            mm.acc_sil = getbits(me, 51, 52)
            mm.acc_sil_type = SIL_PER_SAMPLE if getbit(me, 55) else SIL_PER_HOUR
            mm.ops_hrd = HEADING_MAGNETIC if getbit(me, 54) else HEADING_TRUE
            if mm.mesub == 0:
                mm.acc_gva_valid = 1
                mm.acc_gva = getbits(me, 49, 50)
                mm.acc_nic_baro_valid = 1
                mm.acc_nic_baro = getbit(me, 53)
            else:
                mm.ops_tah = mm.ops_hrd if getbit(me, 53) else HEADING_GROUND_TRACK


def decodeExtendedSquitter(mm, me):
    metype = mm.metype = getbits(me, 1, 5)
    check_imf = 0
    if mm.msgtype == 18:
        if mm.CF == 0:
            mm.addrtype = ADDR_ADSB_ICAO_NT
        elif mm.CF == 1:
            mm.addrtype = ADDR_ADSB_OTHER
            mm.addr |= MODES_NON_ICAO_ADDRESS
        elif mm.CF == 2:
            mm.source = SOURCE_TISB
            mm.addrtype = ADDR_TISB_ICAO
            check_imf = 1
        elif mm.CF == 3:
            mm.source = SOURCE_TISB
            mm.addrtype = ADDR_TISB_ICAO
            if getbit(me, 1):
                setIMF(mm)
            return
        elif mm.CF == 5:
            mm.addrtype = ADDR_TISB_OTHER
            mm.source = SOURCE_TISB
            mm.addr |= MODES_NON_ICAO_ADDRESS
        elif mm.CF == 6:
            mm.addrtype = ADDR_ADSR_ICAO
            mm.source = SOURCE_ADSR
            check_imf = 1
        else:
            mm.addrtype = ADDR_UNKNOWN
            mm.addr |= MODES_NON_ICAO_ADDRESS
            return
    if metype in (1, 2, 3, 4):
        decodeESIdentAndCategory(mm, me)
    elif metype == 19:
        decodeESAirborneVelocity(mm, me, check_imf)
    elif metype in (5, 6, 7, 8):
        decodeESSurfacePosition(mm, me, check_imf)
    elif metype in (0, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22):
        decodeESAirbornePosition(mm, me, check_imf)
    elif metype == 23:
        decodeESTestMessage(mm, me)
    elif metype == 24:
        pass
    elif metype == 28:
        decodeESAircraftStatus(mm, me, check_imf)
    elif metype == 29:
        decodeESTargetStatus(mm, me, check_imf)
    elif metype == 30:
        pass
    elif metype == 31:
        decodeESOperationalStatus(mm, me, check_imf)


# ------------------------------------------------------------------------------------- comm_b.c, one MB field per element
def mb_bits(mb, firstbit, lastbit):
    """getbits over an array of 56-bit MB fields held as uint64"""
    return ((mb >> np.uint64(56 - lastbit)) & np.uint64((1 << (lastbit - firstbit + 1)) - 1)).astype(np.int64)


def mb_bit(mb, bit):
    return mb_bits(mb, bit, bit) != 0


class Score:
    """`int score` of one decoder over the array: add() under a mask, dead() for a `return 0`"""

    def __init__(self, n):
        self.score = np.zeros(n, dtype=np.int64)
        self.alive = np.ones(n, dtype=bool)

    def add(self, mask, k):
        self.score += np.where(mask, k, 0)

    def dead(self, mask):
        self.alive &= ~mask

    def result(self):
        return np.where(self.alive, self.score, 0)


def decodeEmptyResponse(mb):
    s = Score(len(mb))
    s.dead(mb != 0)
    s.add(True, 56)
    return s.result(), dict(commb_format=COMMB_EMPTY_RESPONSE)


def decodeBDS10(mb):
    s = Score(len(mb))
    s.dead(mb_bits(mb, 1, 8) != 0x10)
    s.dead(mb_bits(mb, 10, 14) != 0)
    s.add(True, 56)
    return s.result(), dict(commb_format=COMMB_DATALINK_CAPS)


def decodeBDS17(mb):
    s = Score(len(mb))
    s.dead(mb_bits(mb, 25, 56) != 0)
    s.add(mb_bit(mb, 7), 1)
    s.add(~mb_bit(mb, 7), -2)
    for unlikely in (10, 11, 12, 13, 14, 20, 21, 22):
        s.add(mb_bit(mb, unlikely), -2)
    b = [None] + [mb_bit(mb, i) for i in range(1, 7)]
    es = b[1] & b[2] & b[3] & b[4] & b[5]
    no_es = ~b[1] & ~b[2] & ~b[3] & ~b[4] & ~b[5] & ~b[6]
    s.add(es, 5)
    s.add(es & b[6], 1)
    s.add(~es & no_es, 1)
    s.add(~es & ~no_es, -12)
    both = mb_bit(mb, 16) & mb_bit(mb, 24)
    neither = ~mb_bit(mb, 16) & ~mb_bit(mb, 24) & ~mb_bit(mb, 9)
    s.add(both, 2)
    s.add(both & mb_bit(mb, 9), 1)
    s.add(~both & neither, 1)
    s.add(~both & ~neither, -6)
    return s.result(), dict(commb_format=COMMB_GICB_CAPS)


def decodeBDS20(mb):
    s = Score(len(mb))
    s.dead(mb_bits(mb, 1, 8) != 0x20)
    chars = np.stack([mb_bits(mb, 9 + 6 * i, 14 + 6 * i) for i in range(8)], axis=1)
    callsign = np.frombuffer(ais_charset, dtype=np.uint8)[chars]
    s.add(True, 8)
    valid = np.ones(len(mb), dtype=bool)
    for i in range(8):
        c = callsign[:, i]
        good = ((c >= ord("A")) & (c <= ord("Z"))) | ((c >= ord("0")) & (c <= ord("9"))) | (c == ord(" "))
        s.add(good, 6)
        padding = ~good & (c == ord("@"))
        valid &= ~padding
        s.dead(~good & ~padding)
    return s.result(), dict(commb_format=COMMB_AIRCRAFT_IDENT, callsign_store=valid, callsign=callsign, callsign_valid=valid)


def decodeBDS30(mb):
    s = Score(len(mb))
    s.dead(mb_bits(mb, 1, 8) != 0x30)
    s.add(True, 56)
    return s.result(), dict(commb_format=COMMB_ACAS_RA)


def decodeBDS40(mb):
    n = len(mb)
    mcp_valid, mcp_raw = mb_bit(mb, 1), mb_bits(mb, 2, 13)
    fms_valid, fms_raw = mb_bit(mb, 14), mb_bits(mb, 15, 26)
    baro_valid, baro_raw = mb_bit(mb, 27), mb_bits(mb, 28, 39)
    reserved_1 = mb_bits(mb, 40, 47)
    mode_valid, mode_raw = mb_bit(mb, 48), mb_bits(mb, 49, 51)
    reserved_2 = mb_bits(mb, 52, 53)
    source_valid, source_raw = mb_bit(mb, 54), mb_bits(mb, 55, 56)
    s = Score(n)
    s.dead(~mcp_valid & ~fms_valid & ~baro_valid & ~mode_valid & ~source_valid)

    def altitude(valid, raw):
        first = valid & (raw != 0)
        alt = np.where(first, raw * 16, 0)
        s.add(first & (alt >= 1000) & (alt <= 50000), 13)
        s.dead(first & ~((alt >= 1000) & (alt <= 50000)))  # unlikely altitude
        second = ~first & ~valid & (raw == 0)
        s.add(second, 1)
        s.dead(~first & ~second)
        return alt

    mcp_alt = altitude(mcp_valid, mcp_raw)
    fms_alt = altitude(fms_valid, fms_raw)
    first = baro_valid & (baro_raw != 0)
    baro_setting = np.where(first, (800 + baro_raw * 0.1).astype(f32), f32(0))  # a float
    s.add(first & (baro_setting >= 900) & (baro_setting <= 1100), 13)
    s.dead(first & ~((baro_setting >= 900) & (baro_setting <= 1100)))
    second = ~first & ~baro_valid & (baro_raw == 0)
    s.add(second, 1)
    s.dead(~first & ~second)
    s.dead(reserved_1 != 0)
    s.add(mode_valid, 4)
    s.add(~mode_valid & (mode_raw == 0), 1)
    s.dead(~mode_valid & (mode_raw != 0))
    s.dead(reserved_2 != 0)
    s.add(source_valid, 3)
    s.add(~source_valid & (source_raw == 0), 1)
    s.dead(~source_valid & (source_raw != 0))
    s.add(mcp_valid & fms_valid & (mcp_alt != fms_alt), -4)
    for valid, alt in ((mcp_valid, mcp_alt), (fms_valid, fms_alt)):
        remainder = alt % 500
        s.add(valid & ~((remainder < 16) | (remainder > 484)), -4)
    altitude_source = np.where(source_valid, np.array([NAV_ALT_UNKNOWN, NAV_ALT_AIRCRAFT, NAV_ALT_MCP, NAV_ALT_FMS])[source_raw],
                               NAV_ALT_INVALID)
    modes = (np.where(mode_raw & 4, NAV_MODE_VNAV, 0) | np.where(mode_raw & 2, NAV_MODE_ALT_HOLD, 0) |
             np.where(mode_raw & 1, NAV_MODE_APPROACH, 0))
    store = dict(commb_format=COMMB_VERTICAL_INTENT,
                 nav_mcp_altitude_store=mcp_valid, nav_mcp_altitude_valid=1, nav_mcp_altitude=mcp_alt,
                 nav_fms_altitude_store=fms_valid, nav_fms_altitude_valid=1, nav_fms_altitude=fms_alt,
                 nav_qnh_store=baro_valid, nav_qnh_valid=1, nav_qnh=baro_setting, raw_qnh=baro_raw, raw_qnh_commb=1,
                 nav_modes_store=mode_valid, nav_modes_valid=1, nav_modes=modes,
                 nav_altitude_source=altitude_source)
    return s.result(), store


def decodeBDS50(mb, detail=None):
    n = len(mb)
    roll_valid, roll_sign, roll_raw = mb_bit(mb, 1), mb_bit(mb, 2), mb_bits(mb, 3, 11)
    track_valid, track_sign, track_raw = mb_bit(mb, 12), mb_bit(mb, 13), mb_bits(mb, 14, 23)
    gs_valid, gs_raw = mb_bit(mb, 24), mb_bits(mb, 25, 34)
    track_rate_valid, track_rate_sign, track_rate_raw = mb_bit(mb, 35), mb_bit(mb, 36), mb_bits(mb, 37, 45)
    tas_valid, tas_raw = mb_bit(mb, 46), mb_bits(mb, 47, 56)
    s = Score(n)
    s.dead(~roll_valid | ~track_valid | ~gs_valid | ~tas_valid)

    roll = (roll_raw * 45.0 / 256.0).astype(f32)
    roll = np.where(roll_sign, (roll.astype(np.float64) - 90.0).astype(f32), roll)
    roll = np.where(roll_valid, roll, f32(0))
    ok = (roll >= -40) & (roll < 40)
    s.add(roll_valid & ok, 11)
    s.dead(roll_valid & ~ok)
    second = ~roll_valid & (roll_raw == 0) & ~roll_sign
    s.add(second, 1)
    s.dead(~roll_valid & ~second)

    track = (track_raw * 90.0 / 512.0).astype(f32)
    track = np.where(track_sign, (track.astype(np.float64) + 180.0).astype(f32), track)
    track = np.where(track_valid, track, f32(0))
    s.add(track_valid, 12)
    second = ~track_valid & (track_raw == 0) & ~track_sign
    s.add(second, 1)
    s.dead(~track_valid & ~second)

    def speed(valid, raw):
        first = valid & (raw != 0)
        v = np.where(first, raw * 2, 0)
        s.add(first & (v >= 50) & (v <= 700), 11)
        s.dead(first & ~((v >= 50) & (v <= 700)))
        second = ~first & ~valid & (raw == 0)
        s.add(second, 1)
        s.dead(~first & ~second)
        return v

    gs = speed(gs_valid, gs_raw)

    track_rate = (track_rate_raw * 8.0 / 256.0).astype(f32)
    track_rate = np.where(track_rate_sign, track_rate - f32(16), track_rate).astype(f32)
    track_rate = np.where(track_rate_valid, track_rate, f32(0))
    ok = (track_rate >= -10.0) & (track_rate <= 10.0)
    s.add(track_rate_valid & ok, 11)
    s.dead(track_rate_valid & ~ok)
    second = ~track_rate_valid & (track_rate_raw == 0) & ~track_rate_sign
    s.add(second, 1)
    s.dead(~track_rate_valid & ~second)

    tas = speed(tas_valid, tas_raw)

    # "small penalty for inconsistent data": the difference of the two valid bits, never above 150 (comm_b.c:545-550)
    delta = np.abs(gs_valid.astype(np.int64) - tas_valid.astype(np.int64))
    s.add(gs_valid & tas_valid & (delta > 150), -6)

    # the theoretical turn rate against the track angle rate (comm_b.c:552-559)
    checked = roll_valid & tas_valid & (tas > 0) & track_rate_valid
    with np.errstate(divide="ignore", invalid="ignore"):
        turn_rate = 68625 * np.tan(roll.astype(np.float64) * M_PI / 180.0) / (tas * 20 * M_PI)
        delta = np.abs(turn_rate - track_rate.astype(np.float64))
    s.add(checked & (delta > 2.0), -6)
    if detail is not None:
        detail.update(delta=delta, checked=checked)

    store = dict(commb_format=COMMB_TRACK_TURN,
                 roll_store=roll_valid, roll_valid=1, roll=roll, raw_roll=roll_raw - 512 * roll_sign,
                 heading_store=track_valid, heading_valid=1, heading=track, heading_type=HEADING_GROUND_TRACK,
                 raw_heading=track_raw + 1024 * track_sign,
                 gs_store=gs_valid, gs_valid=1, gs_v0=gs.astype(f32), gs_v2=gs.astype(f32), gs_selected=gs.astype(f32), raw_gs=gs,
                 track_rate_store=track_rate_valid, track_rate_valid=1, track_rate=track_rate,
                 raw_track_rate=track_rate_raw - 512 * track_rate_sign,
                 tas_store=tas_valid, tas_valid=1, tas=tas)
    return s.result(), store


def decodeBDS60(mb):
    n = len(mb)
    heading_valid, heading_sign, heading_raw = mb_bit(mb, 1), mb_bit(mb, 2), mb_bits(mb, 3, 12)
    ias_valid, ias_raw = mb_bit(mb, 13), mb_bits(mb, 14, 23)
    mach_valid, mach_raw = mb_bit(mb, 24), mb_bits(mb, 25, 34)
    baro_rate_valid, baro_rate_sign, baro_rate_raw = mb_bit(mb, 35), mb_bit(mb, 36), mb_bits(mb, 37, 45)
    inertial_rate_valid, inertial_rate_sign, inertial_rate_raw = mb_bit(mb, 46), mb_bit(mb, 47), mb_bits(mb, 48, 56)
    s = Score(n)
    s.dead(~heading_valid | ~ias_valid | ~mach_valid | (~baro_rate_valid & ~inertial_rate_valid))

    heading = (heading_raw * 90.0 / 512.0).astype(f32)
    heading = np.where(heading_sign, (heading.astype(np.float64) + 180.0).astype(f32), heading)
    heading = np.where(heading_valid, heading, f32(0))
    s.add(heading_valid, 12)
    second = ~heading_valid & (heading_raw == 0) & ~heading_sign
    s.add(second, 1)
    s.dead(~heading_valid & ~second)

    first = ias_valid & (ias_raw != 0)
    ias = np.where(first, ias_raw, 0)
    s.add(first & (ias >= 50) & (ias <= 700), 11)
    s.dead(first & ~((ias >= 50) & (ias <= 700)))
    second = ~first & ~ias_valid & (ias_raw == 0)
    s.add(second, 1)
    s.dead(~first & ~second)

    first = mach_valid & (mach_raw != 0)
    mach = np.where(first, (mach_raw * 2.048 / 512).astype(f32), f32(0))
    ok = (mach.astype(np.float64) >= 0.1) & (mach.astype(np.float64) <= 0.9)  # a float against double constants
    s.add(first & ok, 11)
    s.dead(first & ~ok)
    second = ~first & ~mach_valid & (mach_raw == 0)
    s.add(second, 1)
    s.dead(~first & ~second)

    def rate(valid, sign, raw):
        r = raw * 32
        r = np.where(sign, r - 16384, r)
        r = np.where(valid, r, 0)
        ok = (r >= -6000) & (r <= 6000)
        s.add(valid & ok, 11)
        s.dead(valid & ~ok)
        second = ~valid & (raw == 0)  # the sign bit is not looked at
        s.add(second, 1)
        s.dead(~valid & ~second)
        return r

    baro_rate = rate(baro_rate_valid, baro_rate_sign, baro_rate_raw)
    inertial_rate = rate(inertial_rate_valid, inertial_rate_sign, inertial_rate_raw)
    delta = np.abs(baro_rate - inertial_rate)
    s.add(baro_rate_valid & inertial_rate_valid & (delta > 2000), -12)

    store = dict(commb_format=COMMB_HEADING_SPEED,
                 heading_store=heading_valid, heading_valid=1, heading=heading, heading_type=HEADING_MAGNETIC,
                 raw_heading=heading_raw + 1024 * heading_sign,
                 ias_store=ias_valid, ias_valid=1, ias=ias,
                 mach_store=mach_valid, mach_valid=1, mach=mach, raw_mach=mach_raw,
                 baro_rate_store=baro_rate_valid, baro_rate_valid=1, baro_rate=baro_rate,
                 geom_rate_store=inertial_rate_valid, geom_rate_valid=1, geom_rate=inertial_rate)
    return s.result(), store


comm_b_decoders = (decodeEmptyResponse, decodeBDS10, decodeBDS20, decodeBDS30, decodeBDS17, decodeBDS40, decodeBDS50, decodeBDS60)

# which `if (x_valid)` of a decoder's store block guards which members
STORE_GROUPS = {
    "callsign_store": ("callsign", "callsign_valid"),
    "nav_mcp_altitude_store": ("nav_mcp_altitude_valid", "nav_mcp_altitude"),
    "nav_fms_altitude_store": ("nav_fms_altitude_valid", "nav_fms_altitude"),
    "nav_qnh_store": ("nav_qnh_valid", "nav_qnh", "raw_qnh", "raw_qnh_commb"),
    "nav_modes_store": ("nav_modes_valid", "nav_modes"),
    "roll_store": ("roll_valid", "roll", "raw_roll"),
    "heading_store": ("heading_valid", "heading", "heading_type", "raw_heading"),
    "gs_store": ("gs_valid", "gs_v0", "gs_v2", "gs_selected", "raw_gs"),
    "track_rate_store": ("track_rate_valid", "track_rate", "raw_track_rate"),
    "tas_store": ("tas_valid", "tas"),
    "ias_store": ("ias_valid", "ias"),
    "mach_store": ("mach_valid", "mach", "raw_mach"),
    "baro_rate_store": ("baro_rate_valid", "baro_rate"),
    "geom_rate_store": ("geom_rate_valid", "geom_rate"),
}


def decodeCommB(mb, DR, UM, correctedbits, detail=None):
    """comm_b.c:50-84 over arrays: -> {member: (mask of the records it is stored in, values)}.  detail, a dict, receives
    the scores and the turn-rate check's delta."""
    n = len(mb)
    skip = (DR != 0) | (UM != 0) | (correctedbits > 0)
    bestScore = np.zeros(n, dtype=np.int64)
    bestDecoder = np.full(n, -1, dtype=np.int64)
    ambiguous = np.zeros(n, dtype=bool)
    stores, scores = [], []
    for i, decoder in enumerate(comm_b_decoders):
        score, store = decoder(mb, detail) if decoder is decodeBDS50 else decoder(mb)
        better = score > bestScore
        same = ~better & (score == bestScore)
        bestScore = np.where(better, score, bestScore)
        bestDecoder = np.where(better, i, bestDecoder)
        ambiguous = np.where(better, False, ambiguous | same)
        stores.append(store)
        scores.append(score)
    if detail is not None:
        detail.update(scores=np.stack(scores, axis=1), bestDecoder=bestDecoder, ambiguous=ambiguous)
    out = {"commb_format": (np.ones(n, dtype=bool), np.full(n, COMMB_UNKNOWN, dtype=np.int64))}

    def put(name, mask, values):
        if name not in out:
            dt = "S8" if name == "callsign" else (np.float64 if name in FLOAT_MEMBERS else np.int64)
            out[name] = (np.zeros(n, dtype=bool), np.zeros(n, dtype=dt))
        m, v = out[name]
        if name == "callsign":
            values = np.ascontiguousarray(values).view("S8").reshape(n)
        v[mask] = np.broadcast_to(values, (n,))[mask]
        m |= mask

    has = ~skip & (bestDecoder >= 0)
    put("commb_format", has & ambiguous, COMMB_AMBIGUOUS)
    for i, store in enumerate(stores):
        chosen = has & ~ambiguous & (bestDecoder == i)
        guarded = {m: g for g, ms in STORE_GROUPS.items() for m in ms}
        for name, values in store.items():
            if name.endswith("_store"):
                continue
            mask = chosen & store[guarded[name]] if name in guarded else chosen
            put(name, mask, values)
    return out


# ----------------------------------------------------------------------------------------------------- mode_s.c:557-715
ADDRESS_PARITY = (0, 4, 5, 16, 24, 25, 26, 27, 28, 29, 30, 31)


def decodeModesMessage(mm, msgtype, addr, raw, commb):
    """What follows the CRC switch.  raw: the message's bytes; commb(mm): the call of decodeCommB at :669."""
    msg = bits_of(raw)
    mm.msgtype = msgtype
    mm.addr = addr
    if msgtype in ADDRESS_PARITY or msgtype in (20, 21):  # :446-466,533-545
        mm.source, mm.source_known = SOURCE_MODE_S, 1
    elif msgtype == 11:  # :500
        mm.source, mm.source_known = SOURCE_MODE_S_CHECKED, 1
    elif msgtype in (17, 18):  # :529
        mm.source, mm.source_known = SOURCE_ADSB, 1
    if msgtype in (0, 4, 16, 20):
        mm.AC = getbits(msg, 20, 32)
        if mm.AC:
            mm.altitude_baro, mm.altitude_baro_unit = decodeAC13Field(mm.AC)
            if mm.altitude_baro != INVALID_ALTITUDE:
                mm.altitude_baro_valid = 1
    if msgtype in (11, 17):
        mm.CA = getbits(msg, 6, 8)
        if mm.CA == 0:
            mm.airground = AG_UNCERTAIN
        elif mm.CA == 4:
            mm.airground = AG_GROUND
        elif mm.CA == 5:
            mm.airground = AG_AIRBORNE
        elif mm.CA == 6:
            mm.airground = AG_UNCERTAIN
        elif mm.CA == 7:
            mm.airground = AG_UNCERTAIN
    if msgtype == 0:
        mm.CC = getbit(msg, 7)
    if msgtype == 18:
        mm.CF = getbits(msg, 6, 8)
    if msgtype in (4, 5, 20, 21):
        mm.DR = getbits(msg, 9, 13)
    if msgtype in (4, 5, 20, 21):
        mm.FS = getbits(msg, 6, 8)
        mm.alert_valid = 1
        mm.spi_valid = 1
        if mm.FS == 0:
            mm.airground = AG_UNCERTAIN
        elif mm.FS == 1:
            mm.airground = AG_GROUND
        elif mm.FS == 2:
            mm.airground = AG_UNCERTAIN
            mm.alert = 1
        elif mm.FS == 3:
            mm.airground = AG_GROUND
            mm.alert = 1
        elif mm.FS == 4:
            mm.airground = AG_UNCERTAIN
            mm.alert = 1
            mm.spi = 1
        elif mm.FS == 5:
            mm.airground = AG_UNCERTAIN
            mm.spi = 1
        else:
            mm.spi_valid = 0
            mm.alert_valid = 0
    if msgtype in (5, 21):
        mm.ID = getbits(msg, 20, 32)
        if mm.ID:
            mm.squawk = decodeID13Field(mm.ID)
            mm.squawk_valid = 1
    if 24 <= msgtype <= 31:
        mm.KE = getbit(msg, 4)
    if msgtype in (20, 21):
        commb(mm)
    if msgtype in (17, 18):
        decodeExtendedSquitter(mm, bits_of(raw[4:11]))
    if 24 <= msgtype <= 31:
        mm.ND = getbits(msg, 5, 8)
    if msgtype in (0, 16):
        mm.RI = getbits(msg, 14, 17)
    if msgtype in (0, 16):
        mm.SL = getbits(msg, 9, 11)
    if msgtype in (4, 5, 20, 21):
        mm.UM = getbits(msg, 14, 19)
    if msgtype in (0, 16):
        mm.VS = getbit(msg, 6)
        if mm.VS:
            mm.airground = AG_GROUND
        else:
            mm.airground = AG_UNCERTAIN


# ---------------------------------------------------------------------------------------- the reading of a record array
def read(records, detail=None, one_buffer=False):
    """records: an array of the product's message records (msgtype, addr, msg).  -> {member of MEMBERS (and callsign):
    array}, struct modesMessage as the reference leaves it.  one_buffer: the Mode A/C replies are those of one sample
    buffer in order -- demodulate2400AC clears its struct modesMessage once per buffer (demod_2400.c:523-528) and
    decodeModeAMessage assigns the altitude only where the reply has one, so a reply without keeps the last one's."""
    n = len(records)
    msgtype = records["msgtype"].astype(np.int64)
    raw = np.ascontiguousarray(records["msg"])
    cols = {m: np.zeros(n, dtype=np.float64 if m in FLOAT_MEMBERS else np.int64) for m in MEMBERS}
    cols["callsign"] = np.zeros(n, dtype="S8")
    commb_at = np.flatnonzero((msgtype == 20) | (msgtype == 21))
    calls = {}  # record -> (DR, UM, correctedbits) as they are when :669 is reached

    def commb(mm):
        calls[mm.index] = (mm.DR, mm.UM, 0)  # (DF20/21 are never bit-corrected: the switch has no repair for them)

    cache = {}
    mms = []
    buffer_mm = MM()
    for i in range(n):
        t = int(msgtype[i])
        nbytes = 2 if t == 32 else (14 if t & 16 else 7)
        b = raw[i, :nbytes].tobytes()
        key = (t, int(records["addr"][i]), b[:4]) if t in (20, 21) else None
        if key is not None and key in cache:  # the header of a Comm-B reply: everything but the MB field
            calls[i] = calls[cache[key].index]
            mms.append(cache[key])
            continue
        mm = MM()
        mm.index = i
        if t == 32 and one_buffer:
            decodeModeAMessage(buffer_mm, (b[0] << 8) | b[1])
            mm.__dict__.update(buffer_mm.__dict__)
        elif t == 32:
            decodeModeAMessage(mm, (b[0] << 8) | b[1])
        else:
            decodeModesMessage(mm, t, int(records["addr"][i]), b, commb)
        if key is not None:
            cache[key] = mm
        mms.append(mm)
    for m in MEMBERS:
        cols[m][:] = [getattr(mm, m) for mm in mms]
    cols["callsign"][:] = [mm.callsign for mm in mms]
    if len(commb_at):
        mb = np.zeros(len(commb_at), dtype=np.uint64)
        for k in range(7):
            mb = (mb << np.uint64(8)) | raw[commb_at, 4 + k].astype(np.uint64)
        state = np.array([calls[int(i)] for i in commb_at], dtype=np.int64).reshape(-1, 3)
        for name, (mask, values) in decodeCommB(mb, state[:, 0], state[:, 1], state[:, 2], detail).items():
            cols[name][commb_at[mask]] = values[mask]
    return cols


def members_of(cols):
    """struct modesMessage columns -> the product's members (FIELD_NAMES), by the table at the top of this file"""
    c = cols
    o = {}
    for name in ("altitude_baro", "AC", "ID", "squawk", "altitude_baro_valid", "altitude_baro_unit", "squawk_valid", "airground",
                 "alert", "alert_valid", "spi", "spi_valid", "CA", "CC", "CF", "DR", "FS", "KE", "ND", "RI", "SL", "UM", "VS",
                 "source", "addrtype", "addr", "metype", "mesub", "cpr_valid", "cpr_type", "cpr_odd", "callsign_valid",
                 "callsign", "cpr_lat", "cpr_lon", "altitude_geom", "altitude_geom_valid", "altitude_geom_unit", "category",
                 "category_valid", "ias", "tas", "ias_valid", "tas_valid", "baro_rate_valid", "geom_rate_valid", "baro_rate",
                 "geom_rate", "geom_delta", "geom_delta_valid", "emergency_valid", "emergency", "nav_altitude_source",
                 "nav_modes", "nav_heading_type", "nav_mcp_altitude", "nav_fms_altitude", "commb_format"):
        o[name] = c[name]
    o["imf"] = c["imf_set"]
    o["nic_b_valid"], o["nic_b"] = c["acc_nic_b_valid"], c["acc_nic_b"]
    o["nac_v_valid"], o["nac_v"] = c["acc_nac_v_valid"], c["acc_nac_v"]
    o["velocity_valid"], o["ew_vel"], o["ns_vel"] = c["velocity_set"], c["ew_vel"], c["ns_vel"]
    from_velocity = c["velocity_set"] != 0
    o["heading_valid"] = np.where(from_velocity, 0, c["heading_valid"])
    o["heading_type"] = np.where(from_velocity, 0, c["heading_type"])
    o["heading_raw"] = c["raw_heading"]
    o["movement"] = c["raw_movement"]
    o["nav_valid"] = (c["nav_modes_valid"] | c["nav_heading_valid"] << 1 | c["nav_mcp_altitude_valid"] << 2 |
                      c["nav_fms_altitude_valid"] << 3 | c["nav_qnh_valid"] << 4 | c["raw_nav_heading_v2"] << 5 |
                      c["raw_qnh_commb"] << 6)
    o["acc_valid"] = (c["acc_nac_p_valid"] | c["acc_nic_baro_valid"] << 1 | c["acc_nic_a_valid"] << 2 |
                      c["acc_nic_c_valid"] << 3 | c["acc_gva_valid"] << 4 | c["acc_sda_valid"] << 5)
    for name in ("nac_p", "nic_baro", "nic_a", "nic_c", "gva", "sda", "sil", "sil_type"):
        o[name] = c["acc_" + name]
    o["cc_antenna_offset"] = c["ops_cc_antenna_offset"]
    o["nav_heading_raw"], o["nav_qnh_raw"] = c["raw_nav_heading"], c["raw_qnh"]
    o["opstatus"] = (c["ops_valid"] | c["ops_version"] << 1 | c["ops_om_acas_ra"] << 4 | c["ops_om_ident"] << 5 |
                     c["ops_om_atc"] << 6 | c["ops_om_saf"] << 7 | c["ops_cc_acas"] << 8 | c["ops_cc_cdti"] << 9 |
                     c["ops_cc_1090_in"] << 10 | c["ops_cc_arv"] << 11 | c["ops_cc_ts"] << 12 | c["ops_cc_tc"] << 13 |
                     c["ops_cc_uat_in"] << 15 | c["ops_cc_poa"] << 16 | c["ops_cc_b2_low"] << 17 | c["ops_cc_lw_valid"] << 18 |
                     c["ops_cc_lw"] << 19 | c["ops_hrd"] << 23 | c["ops_tah"] << 26)
    o["roll_q"], o["track_rate_q"], o["gs"], o["mach_raw"] = c["raw_roll"], c["raw_track_rate"], c["raw_gs"], c["raw_mach"]
    gs_commb = c["gs_valid"] & (c["commb_format"] == COMMB_TRACK_TURN)
    o["commb_valid"] = (c["roll_valid"] | gs_commb << 1 | c["track_rate_valid"] << 2 | c["mach_valid"] << 3)
    assert set(o) == set(FIELD_NAMES), set(o) ^ set(FIELD_NAMES)
    return o, c["source_known"] != 0


def floats_of(cols):
    """the float-valued members, in the layout of msd_fields_float (FLOAT_NAMES): float, mach widened to double"""
    c = cols
    o = {name: c[name].astype(np.float32) for name in ("gs_v0", "gs_v2", "gs_selected", "heading", "track_rate", "roll",
                                                       "nav_qnh", "nav_heading")}
    o["mach"] = c["mach"].astype(np.float32).astype(np.float64)
    for name in ("gs_valid", "heading_valid", "heading_type", "track_rate_valid", "roll_valid", "mach_valid", "nav_qnh_valid",
                 "nav_heading_valid"):
        o[name] = c[name]
    assert set(o) == set(FLOAT_NAMES)
    return o
