"""Endpoint groups (include/ggrs_amd.h rb_decode_input_packets_grouped,
rb_encode_input_packets_grouped): the handles whose
inputs one endpoint carries in one stream.

A remote peer with several local players sends all of them in one Input
message (InputBytes::from_inputs, network/protocol.rs:61-79), and a spectator
endpoint carries every player of the match.  Such an endpoint owns the row of
its lowest handle, the lead, in every [P, S] endpoint tensor; the datagram,
protocol and liveness calls serve it under ``lead_mask``, and ``spread`` hands
what they report for the lead to the group's other handles.
"""
from __future__ import annotations


class EndpointGroups:
    """groups: a sequence of handle sequences or handle masks, up to four, none empty, no handle
    twice, every handle below num_players."""

    def __init__(self, groups, num_players: int):
        P = int(num_players)
        if not 1 <= P <= 4:
            raise ValueError("one to four players")
        masks = []
        for g in groups:
            if isinstance(g, int):
                m = g
            else:
                m = 0
                for h in g:
                    h = int(h)
                    if h < 0 or (m >> h) & 1:
                        raise ValueError("a group names a handle once, from 0 up")
                    m |= 1 << h
            if m <= 0 or m >> P:
                raise ValueError("a group is a non-empty set of handles below num_players")
            if any(m & o for o in masks):
                raise ValueError("two groups share a handle")
            masks.append(m)
        if not 1 <= len(masks) <= 4:
            raise ValueError("one to four groups")
        self.num_players = P
        self.masks = tuple(masks)

    @classmethod
    def spectator(cls, num_players: int) -> "EndpointGroups":
        """The single group of all handles: what a host sends a spectator
        (send_confirmed_inputs_to_spectators, sessions/p2p_session.rs:676-703)."""
        return cls([(1 << int(num_players)) - 1], num_players)

    @property
    def packed(self) -> int:
        """The uint32 group_masks of the C calls: byte g is group g's handle mask."""
        return sum(m << (8 * g) for g, m in enumerate(self.masks))

    @property
    def leads(self):
        return tuple((m & -m).bit_length() - 1 for m in self.masks)

    @property
    def lead_mask(self) -> int:
        """The handle_mask of the groups' endpoints for parse, build, protocol and liveness calls."""
        return sum(1 << h for h in self.leads)

    def members(self, lead: int):
        """The handles of the group whose lead is `lead`, ascending."""
        for m, h in zip(self.masks, self.leads):
            if h == int(lead):
                return tuple(i for i in range(self.num_players) if (m >> i) & 1)
        raise KeyError(f"no group is led by handle {lead}")

    def spread(self, t):
        """Copy each lead's row of a [..., P, S] tensor onto the rows of its group's other handles,
        in place, and return t: the endpoint's `received` byte, disconnect_requested and peer
        status for every handle it carries (one endpoint timer disconnects every handle of the
        endpoint, p2p_session.rs:835-844).  Does not synchronise."""
        assert t.shape[-2] == self.num_players
        for lead in self.leads:
            rest = self.members(lead)[1:]
            if rest:
                row = t[..., lead:lead + 1, :]
                t[..., list(rest), :] = row.clone() if hasattr(row, "clone") else row.copy()
        return t

    def __repr__(self):
        return f"EndpointGroups({[list(self.members(h)) for h in self.leads]}, num_players={self.num_players})"


def as_groups(groups, num_players: int) -> EndpointGroups:
    return groups if isinstance(groups, EndpointGroups) else EndpointGroups(groups, num_players)
